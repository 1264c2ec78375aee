/*
 * onet_hip_verify.h -- C ABI of libonet_hip.so, the performance report's device side: what verify_onet_simclutter's second loop
 * (measure_snr_on_fg, TS:46-95, with get_psnr, UT:457-476) and the two-stage cascade (test_2nd_stage_simclutter, TS:296-418) do
 * with the forward's Vt, Vd besides counting -- per-frame min / max, the sums and maxima get_psnr is made of, and the batch's
 * flip decision read from the confusion counts the batch has just produced, on the device.  The conventions are
 * onet_hip_eval.h's (device pointers, enqueue only, 0 / negative ONET_E* codes with onet_last_error(), `stream` a hipStream_t
 * passed as void*; gt read in its own dtype by the same codes -- 0 uint8 / bool, 1 int32, 2 int64, 3 float32 -- image b at
 * gt + b * gt_bs elements, positive where != 0; 16-byte loads where HW % 4 == 0 and every pointer and batch stride is aligned for
 * them, scalar loads elsewhere; B <= 65535).  The entry points live in a header of their own so that the others keep their sets.
 *
 * n(v) = (v - lo) / ((hi - lo) + spacing(1)) in fp32, lo / hi the frame's min / max: onet_normalise_per_frame's expression, one
 * __device__ function shared by the three kernels (tensor_normal_per_frame, UT:673-689).
 *
 * onet_snr_moments: Vt, Vd [B][HW] fp32 contiguous; X fp32, image b at X + b * x_bs (x_bs >= HW), or NULL.  Writes
 *   minmax[b][4] = (min Vt, max Vt, min Vd, max Vd) fp32 and WRITES (does not add to) the fp64 row moments[b][9] = for each
 *   source s of (X as it is, n(Vt), n(Vd)): moments[b][3 s + 0] = sum of v^2 over the pixels with gt != 0, [3 s + 1] = sum of v^2
 *   over the pixels with gt == 0, [3 s + 2] = max(0, max of v over the pixels with gt != 0).  Each square is formed in fp64 from
 *   the fp32 value and the sums are fp64.  X == NULL: the three X values are written as 0.  No floating-point atomics: block g
 *   of an image's G = min(ceil(HW / 1024), 64) blocks takes the 1024-pixel chunks g, g + G, ..., the blocks' partial results go
 *   to `ws` and are merged in one fixed order, so an image's row has the same bits in every run.  ws: 8-byte aligned,
 *   ws_bytes >= B * 64 * 88 (per image and block 9 doubles and 4 floats).
 * onet_cascade_input: X2[b] = n(flip ? Vt[b] : Vd[b]), X2 [B][HW] fp32 contiguous.  counts: the batch's B int64 rows
 *   (TP, FP, FN, TN) as onet_score_counts left them; every block sums them itself: flip = (sum TP + sum TN) < (sum FP + sum FN),
 *   integers (re_assign_label's pred_acc < reor_acc, UT:439-453; a tie keeps the labels, and unchanged labels make Vd the
 *   foreground, TS:327-332).  minmax: onet_snr_moments' [B][4], or NULL: the kernel finds the selected frame's min / max itself.
 */
#ifndef ONET_HIP_VERIFY_H
#define ONET_HIP_VERIFY_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_snr_moments(const float* X, int64_t x_bs, const float* Vt, const float* Vd, const void* gt, int gt_dtype, int64_t gt_bs,
                     double* moments, float* minmax, int B, int HW, void* ws, int64_t ws_bytes, void* stream);
int onet_cascade_input(const float* Vt, const float* Vd, const float* minmax, const int64_t* counts, float* X2, int B, int HW,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_VERIFY_H */
