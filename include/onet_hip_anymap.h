/*
 * onet_hip_anymap.h -- C ABI of libonet_hip.so, the one-part (plain bf16) eval plan on maps of ANY size below its first level:
 * 200 x 200 pools to 100, 50 (W % 4 == 2) and 25 pixels (odd), which onet_hip_ragged.h's domain (even H, W % 4 == 0) does not
 * take.  The conventions are onet_hip.h's; the entry points live in a header of their own, as onet_hip_ragged.h's do, so that
 * the existing headers keep their sets of prototypes.
 *
 * Each entry is its ragged sibling of onet_hip_ragged.h (onet_conv3x3_plain16_fwd_pre_act_ragged / _act_pool_ragged) with the
 * sibling's arguments and this domain:
 *   H, W > 0, H W < 2^24, Cin % 32 == 0, Cout % 64 == 0, inside the 2 GiB buffer-resource range, a_amax NULL.
 * Outside it they return 1: nothing launched, nothing written.  Inside it the valid region holds, value for value, what the
 * full-tile entry writes on the map zero-padded to whole tiles, and nothing outside the map is written.  On a map the ragged
 * sibling takes an entry launches exactly what the sibling launches (on a map made of full tiles: the full-tile instance, and
 * the sibling's 16-byte alignment of fp32 rows applies); on every other map the fp32 outputs `a` and `y` are stored float by
 * float, each under its own guard, and need 4-byte alignment only -- a row of 25 or 50 floats is not 16-byte aligned.
 *
 * _act_pool: the pooled maps are H / 2 x W / 2 rounded DOWN, as nn.MaxPool2d(2) pools: yP [B][Cout/8][H/2][W/2][8],
 * y [B][Cout][H/2][W/2], and the batch-stride checks use those sizes.  A 2 x 2 window that is only partly inside an odd map
 * belongs to no pooled pixel and is written to neither.
 *
 * There are no _head or _plain twins: the first level of a plan keeps onet_hip_ragged.h's domain.
 */
#ifndef ONET_HIP_ANYMAP_H
#define ONET_HIP_ANYMAP_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_conv3x3_plain16_fwd_pre_act_anymap(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                            void* a_amax, float* a, int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream);
int onet_conv3x3_plain16_fwd_pre_act_pool_anymap(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                                 void* a_amax, float* a, int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B,
                                                 int Cin, int Cout, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_ANYMAP_H */
