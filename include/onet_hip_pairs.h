/*
 * onet_hip_pairs.h -- C ABI of libonet_hip.so, the one-part (plain bf16) eval plan's BOTTOM level: maps 16 pixels wide or
 * narrower (256 x 256 pools to 16 x 16, 224 x 224 to 14 x 14, 200 x 200 to 12 x 12), which the predicates of the ragged and
 * any-map plans leave to the fall-back because such a map fills at most half of a 16 x 32 tile.  The conventions are
 * onet_hip.h's; the entry point lives in a header of its own, as onet_hip_anymap.h's do, so that the existing headers keep
 * their sets of prototypes.
 *
 * onet_conv3x3_plain16_fwd_pre_act_pairs is onet_conv3x3_plain16_fwd_pre_act_anymap (same arguments) on IMAGE-PAIR tiles: a
 * tile's 32 pixel columns are two images of the batch side by side, each with its own halo columns in the LDS image, so
 * cdiv(B, 2) cdiv(H, 16) Cout / 64 tiles are walked instead of B cdiv(H, 16) Cout / 64 half-empty ones.  Domain:
 *   H > 0, 0 < W <= 16, Cin % 32 == 0, Cout % 64 == 0, a_amax NULL, an image pair (the batch stride plus one image) inside
 *   the 2 GiB buffer-resource range.
 * Outside it the entry returns 1: nothing launched, nothing written.  Inside it the map holds, value for value, what the
 * any-map entry writes there (the same products added in the same order per pixel, the same epilogue expressions), and
 * nothing outside the map is written: `a` is stored float by float, each under its own guard, and needs 4-byte alignment only
 * (a row of 14 floats is not 16-byte aligned).  B may be odd: the last tile then holds one image.
 *
 * There is no _act_pool, _head, ragged or fp16 (hi | mid) twin: the bottom level has no pool and no head.
 */
#ifndef ONET_HIP_PAIRS_H
#define ONET_HIP_PAIRS_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_conv3x3_plain16_fwd_pre_act_pairs(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                           void* a_amax, float* a, int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_PAIRS_H */
