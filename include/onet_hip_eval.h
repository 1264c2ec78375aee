/*
 * onet_hip_eval.h -- C ABI of libonet_hip.so, the validation step: what a validation loop does with the forward's Vt, Vd
 * (test_simclutter, TS:98-172; test_on_zy3_nail, UZ:151-208; "UT" = source_code/utils_20231218.py) as ONE streaming launch
 * per batch that leaves four integers per image on the device.  The conventions are onet_hip.h's (plain pointers and sizes,
 * device pointers, 0 / negative ONET_E* codes with onet_last_error(), `stream` a hipStream_t passed as void*, enqueue only);
 * the entry points live in a header of their own so that onet_hip.h keeps its set of prototypes.
 *
 * Per-image 2-class confusion counts counts[b][4] = (TP, FP, FN, TN), positive class 1 -- the inputs of _acc / _miou /
 * _target_iou / _detection_rate / _false_alarm_rate (UT:100-192), of re_assign_label (UT:410-453: a permutation of the
 * four) and of _hungarian_match (UT:258-285) -- ADDED to what counts holds: the caller zeroes the buffer once per epoch.
 * Integer sums: the result does not depend on the order of the blocks, two runs give the same bits.
 *
 * Label maps (gt, pred) are read in their own dtype, code 0 uint8 (bool), 1 int32, 2 int64, 3 float32 (the reference's
 * label tensors are float32), positive where != 0 (documented domain {0, 1}), image b at base + b * bs elements, its HW
 * elements contiguous (bs >= HW: a batch slice of a wider tensor is read in place).
 *
 * onet_score_counts: the prediction is the head's label of Vt, Vd [B][HW] (fp32, contiguous), s0, s1 and Y = s1 > s0 by
 *   onet_softmax2_labels' expressions bit for bit (ties and NaN: label 0); S [B][2][HW] and / or Y [B][HW] are stored
 *   where the pointer is not NULL.
 * onet_label_counts: the prediction is a label map like gt.
 * Both take 16-byte loads where HW % 4 == 0 and every pointer (and batch stride) is aligned for them, scalar loads elsewhere;
 * B <= 65535.
 */
#ifndef ONET_HIP_EVAL_H
#define ONET_HIP_EVAL_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_score_counts(const float* Vt, const float* Vd, const void* gt, int gt_dtype, int64_t gt_bs,
                      float* S, int64_t* Y, int64_t* counts, int B, int HW, void* stream);
int onet_label_counts(const void* pred, int pred_dtype, int64_t pred_bs, const void* gt, int gt_dtype, int64_t gt_bs,
                      int64_t* counts, int B, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_EVAL_H */
