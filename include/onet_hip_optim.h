/*
 * onet_hip_optim.h -- C ABI of libonet_hip.so, the optimizer step with its hyper-parameters in DOUBLE, as torch.optim.Adam holds them.
 *
 * onet_adam_step (onet_hip.h) takes float betas, and 1 - beta of a rounded beta is not the rounded 1 - beta: 1 - 0.999f is 1.3e-5
 * (relative) away from 0.001, which the second moment of the first steps carries in full.  This entry forms 1 - beta, lr / (1 - beta1^step)
 * and 1 / sqrt(1 - beta2^step) in double and rounds each once; everything else is onet_adam_step's: the same kernel, one fused launch
 * over the flat buffers, 16-byte aligned pointers required, step 1-based, L2 weight decay, no amsgrad.  Declared in a header of its own:
 * onet_hip.h keeps its prototypes and the ABI its version.
 */
#ifndef ONET_HIP_OPTIM_H
#define ONET_HIP_OPTIM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int onet_adam_step_f64(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int step, float grad_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
