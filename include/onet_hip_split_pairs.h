/*
 * onet_hip_split_pairs.h -- C ABI of libonet_hip.so, the fp32-level (fp16 hi | mid parts) eval plan's BOTTOM level: maps 16 pixels
 * wide or narrower (256 x 256 pools to 16 x 16, 224 x 224 to 14 x 14), which eval_layer_ok_ragged_fp16 leaves to the fall-back because
 * such a map fills at most half of a 16 x 32 tile.  The two-part counterpart of onet_hip_pairs.h, in a header of its own so that every
 * existing header keeps its set of prototypes.  The conventions are onet_hip.h's.
 *
 * onet_conv3x3_split_fwd_pre_act_pairs is onet_conv3x3_split_fwd_pre_act_ragged (same arguments: the operand's magnitude slots
 * x_amax / scale_always / x_amax2 / split_ch, the output's bound aP_slots, the record a_amax) on IMAGE-PAIR tiles: a tile's 32 pixel
 * columns are two images of the batch side by side, each with its own halo columns in the LDS image, so cdiv(B, 2) cdiv(H, 16)
 * Cout / 64 tiles are walked instead of B cdiv(H, 16) Cout / 64 half-empty ones.  Domain:
 *   H > 0, 0 < W <= 16, Cin % 16 == 0, Cout % 64 == 0, an image pair (the batch stride plus one image) inside the 2 GiB
 *   buffer-resource range.
 * Outside it the entry returns 1: nothing launched, nothing written.  Inside it the map holds, value for value, what the ragged entry
 * writes there (on the map zero-padded to that entry's domain: the same products added in the same order per pixel, the same
 * epilogue expressions, the same 2^k), and nothing outside the map is written: every slot and every float of `a` is stored under
 * its own image < B && y < H && x < W guard.  a_amax (may be NULL) receives the exact maximum over the map's pixels of the batch's
 * own images -- bit-equal to the maximum of `a` of the same launch.  B may be odd: the last tile then holds one image, and the
 * accumulators of its absent half -- relu(bn(0)), not zero -- enter neither a store nor the record.
 *
 * There is no _act_pool, _head or _plain twin: the bottom level has no pool and no head.
 */
#ifndef ONET_HIP_SPLIT_PAIRS_H
#define ONET_HIP_SPLIT_PAIRS_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_conv3x3_split_fwd_pre_act_pairs(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                         const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots, void* a_amax, float* a,
                                         int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_SPLIT_PAIRS_H */
