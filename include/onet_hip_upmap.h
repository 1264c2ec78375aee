/*
 * onet_hip_upmap.h -- C ABI of libonet_hip.so, the one-part (plain bf16) eval plan's ConvTranspose2d edges on maps of ANY size:
 * an input map of odd w (25 -> 50) and an output that is padded into an odd concat map (12 -> 24, placed in 25), which the
 * slot-operand entries of onet_hip.h and onet_hip_ragged.h refuse (even w, a dense 2h x 2w output).  The conventions are
 * onet_hip.h's; the entry point lives in a header of its own, as onet_hip_pairs.h's does, so that the existing headers keep
 * their sets of prototypes.
 *
 * onet_convT2x2_fwd_slots_anymap is onet_convT2x2_fwd_slots_ragged (same leading arguments) with the output map's own size:
 * yP is [B][Ct/8][Ho][1][Wo][8], Ho x Wo slots per channel group.  Floor pooling makes the concat map at most one row and one
 * column larger than the up-sampled map, so the reference's F.pad offsets (diff // 2) are 0: the 2h x 2w block goes to rows
 * 0 .. 2h - 1 and columns 0 .. 2w - 1, and the pad strip -- row 2h, column 2w -- is written as all-zero slots by the SAME
 * launch, each slot once.  Domain:
 *   Cin % 32 == 0, Cin >= 128, Ct % 32 == 0, any w > 0, Ho - 2h in {0, 1}, Wo - 2w in {0, 1}, the operands inside the 2 GiB
 *   buffer-resource range; yP_bs (4-byte units) holds Ct/8 groups of Ho x Wo slots.
 * Outside it the entry returns 1: nothing launched, nothing written.  Inside it the 2h x 2w block holds, value for value, what
 * onet_convT2x2_fwd_slots_ragged writes for the same pixels (pixels are independent columns of the GEMM), and nothing outside
 * the Ct/8 groups' Ho x Wo maps is written.  With even w, Ho == 2h and Wo == 2w it launches exactly what that entry launches.
 *
 * There is no fp16 (hi | mid) twin: the any-map plan exists on the one-part format alone.
 */
#ifndef ONET_HIP_UPMAP_H
#define ONET_HIP_UPMAP_H

#include "onet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int onet_convT2x2_fwd_slots_anymap(const void* xP, int64_t xP_bs, const void* wP, const float* bias, void* yP, int64_t yP_bs, int B, int Cin, int Ct,
                                   int h, int w, int Ho, int Wo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONET_HIP_UPMAP_H */
