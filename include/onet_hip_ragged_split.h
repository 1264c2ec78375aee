/*
 * onet_hip_ragged_split.h -- C ABI of libonet_hip.so, the fp32-level (fp16 hi | mid parts) eval plan on RAGGED maps: maps that are
 * not made of full 16 x 32 tiles, such as the data sets' 224 x 224 below its first level (112, 56, 28 pixels) or 200 x 200.  The
 * two-part counterpart of onet_hip_ragged.h, in a header of its own so that every existing header keeps its set of prototypes.  The
 * conventions are onet_hip.h's.
 *
 * Each convolution entry is its full-tile sibling of onet_hip.h (onet_conv3x3_split_fwd_pre_act / _act_pool / _head; _plain:
 * onet_conv3x3_split_fwd_pre with wq_f16 = 1, an fp32 z and no statistics) with the sibling's arguments -- magnitude slots of the
 * operand (x_amax, scale_always, x_amax2, split_ch) and of the output (aP_slots) included -- and this domain:
 *   H even, W % 4 == 0, H W < 2^24, Cin % 16 == 0, Cout % 64 == 0 (_head: Cout == 64), inside the 2 GiB buffer-resource range.
 * Outside it they return 1: nothing launched, nothing dereferenced, nothing written.  Inside it the valid region holds, value for
 * value, what the sibling writes on the map zero-padded to whole tiles (an out-of-map input slot is a bounds-checked load that
 * returns zero), and nothing outside the map is written: every store stands under its own y < H && x < W guard.  On a map made of
 * full tiles an entry launches exactly what its sibling launches.
 *
 * Unlike the one-part entries, _act_ragged and _act_pool_ragged TAKE a_amax: the record is the exact maximum over the MAP's own
 * pixels -- bit-equal to the maximum of the fp32 activation `a` of the same launch.  (The sibling on the zero-padded canvas records
 * the maximum over the canvas: relu(bn(.)) of an out-of-map pixel is not zero.)  The fp16 plan's bounds start from these records.
 *
 * onet_convT2x2_fwd_slots_split_ragged: onet_convT2x2_fwd_slots with nparts = 2 (fp16 hi | mid operands; x_amax / y_amax: the
 * magnitude slots of input and output, guard rule) without h w % 128 == 0: Cin % 32 == 0, Cin >= 128, Ct % 32 == 0, w even.  Pixel
 * tiles are counted per image; a pixel beyond the map reads zero, in both parts, and is not stored.  On a map with h w % 128 == 0 it
 * launches what onet_convT2x2_fwd_slots launches.
 */
#ifndef ONET_HIP_RAGGED_SPLIT_H
#define ONET_HIP_RAGGED_SPLIT_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_conv3x3_split_fwd_pre_plain_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                            const void* wq, float* z, int64_t z_bs, int B, int Cin, int Cout, int H, int W, void* stream);
int onet_conv3x3_split_fwd_pre_act_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                          const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots, void* a_amax, float* a,
                                          int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream);
int onet_conv3x3_split_fwd_pre_act_pool_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2,
                                               int split_ch, const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots,
                                               void* a_amax, float* a, int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B, int Cin,
                                               int Cout, int H, int W, void* stream);
int onet_conv3x3_split_fwd_pre_head_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                           const void* wq, const float* save, const float* L, int64_t L_bs, float* V, int B, int Cin, int Cout,
                                           int H, int W, void* stream);
int onet_convT2x2_fwd_slots_split_ragged(const void* xP, int64_t xP_bs, const void* x_amax, const void* wP, const float* bias, void* yP,
                                         int64_t yP_bs, const void* y_amax, int nparts, int B, int Cin, int Ct, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_RAGGED_SPLIT_H */
