/*
 * onet_hip_ragged.h -- C ABI of libonet_hip.so, the one-part (plain bf16) eval plan on RAGGED maps: maps that are not made of
 * full 16 x 32 tiles, such as the data sets' 224 x 224 below its first level (112, 56, 28 pixels) or 200 x 200.  The conventions
 * are onet_hip.h's; the entry points live in a header of their own, as onet_hip_eval.h's do, so that both existing headers keep
 * their sets of prototypes.
 *
 * Each convolution entry is its full-tile sibling of onet_hip.h (onet_conv3x3_plain16_fwd_pre_act / _act_pool / _head; _plain:
 * onet_conv3x3_split_fwd_pre with wq_f16 = 2, an fp32 z and no statistics) with the sibling's arguments and this domain:
 *   H even, W % 4 == 0 (the float4 accesses of L, z and the fp32 activation), H W < 2^24, Cin % 32 == 0, Cout % 64 == 0
 *   (_head: Cout == 64), inside the 2 GiB buffer-resource range; a_amax must be NULL (the exact-maximum record would see a
 *   tile's out-of-map accumulators).
 * Outside it they return 1: nothing launched, nothing written.  Inside it the valid region holds, value for value, what the
 * sibling writes on the map zero-padded to whole tiles (an out-of-map input slot is a bounds-checked load that returns zero),
 * and nothing outside the map is written: every store stands under its own y < H && x < W guard.  On a map made of full tiles
 * an entry launches exactly what its sibling launches.  With H and W even a 2 x 2 pooling window is wholly inside the map or
 * wholly outside; the pooled maps are H / 2 x W / 2.
 *
 * onet_convT2x2_fwd_slots_ragged: onet_convT2x2_fwd_slots for one-part operands (nparts = 1, no magnitude slots) without
 * h w % 128 == 0: Cin % 32 == 0, Cin >= 128, Ct % 32 == 0, w even.  Pixel tiles are counted per image; a pixel beyond the map
 * reads zero and is not stored.
 */
#ifndef ONET_HIP_RAGGED_H
#define ONET_HIP_RAGGED_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_conv3x3_plain16_fwd_pre_plain_ragged(const void* xs, int64_t xs_bs, const void* wq, float* z, int64_t z_bs, int B, int Cin, int Cout,
                                              int H, int W, void* stream);
int onet_conv3x3_plain16_fwd_pre_act_ragged(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                            void* a_amax, float* a, int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream);
int onet_conv3x3_plain16_fwd_pre_act_pool_ragged(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                                 void* a_amax, float* a, int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B,
                                                 int Cin, int Cout, int H, int W, void* stream);
int onet_conv3x3_plain16_fwd_pre_head_ragged(const void* xs, int64_t xs_bs, const void* wq, const float* save, const float* L, int64_t L_bs,
                                             float* V, int B, int Cin, int Cout, int H, int W, void* stream);
int onet_convT2x2_fwd_slots_ragged(const void* xP, int64_t xP_bs, const void* wP, const float* bias, void* yP, int64_t yP_bs, int B, int Cin, int Ct,
                                   int h, int w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_RAGGED_H */
