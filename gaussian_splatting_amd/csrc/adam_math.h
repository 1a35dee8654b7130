// adam_math.h -- the one definition of the Adam arithmetic, shared by k_adam (train_ops.hip) and the
// per-Gaussian backward that steps its own parameters (preprocess.hip, k_preprocess_bwd<.., .., ADAM>).
// Both translation units are built with -ffp-contract=off: the same expressions give the same bits,
// so gs_preprocess_backward_adam == gs_preprocess_backward followed by gs_adam_step, bit for bit.
#pragma once
#include <math.h>

#include "gs_common.h"

namespace gs {

// torch/optim/adam.py _single_tensor_adam (amsgrad=False, weight_decay=0, maximize=False), with the
// operation order of the ATen CPU kernels:
//   exp_avg.lerp_(grad, 1 - beta1)                         a + w (b - a)         (|w| < 0.5)
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2) self + (value t1) t2
//   denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//   param.addcdiv_(exp_avg, denom, value=-step_size)       self + (value t1) / t2
__device__ inline void adam_update(float& p, float g, float& m, float& v, float w1, float beta2,
                                   float w2, float bc2_sqrt, float eps, float neg_step) {
    m = m + w1 * (g - m);
    v = v * beta2 + (w2 * g) * g;
    const float denom = __builtin_sqrtf(v) / bc2_sqrt + eps;
    p = p + (neg_step * m) / denom;
}

// what one launch shares: torch passes `1 - beta1`, `beta2`, `1 - beta2`, `eps` as Python floats (fp64)
// that the fp32 kernels round once
struct AdamShared {
    float w1, beta2, w2, eps;
};
inline AdamShared adam_shared(double beta1, double beta2, double eps) {
    return AdamShared{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
}

// per tensor (the step counts differ between tensors after an opacity reset).  torch/optim/adam.py: bias
// corrections and the step size are Python floats (fp64), the kernels then take them as fp32 scalars.
// step: the 1-based count AFTER the increment.
inline void adam_scalars(double lr, int64_t step, double beta1, double beta2, float* neg_step_size,
                         float* bc2_sqrt) {
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    *neg_step_size = (float)(-(lr / bc1));   // -lr / (1 - beta1^step)
    *bc2_sqrt = (float)sqrt(bc2);            // sqrt(1 - beta2^step)
}

// 16-byte accesses that bypass the vector L1 (a value streamed through once per training iteration)
typedef float vfloat4 __attribute__((ext_vector_type(4)));
__device__ inline float4 nt_load4(const float* p) {
    const vfloat4 v = __builtin_nontemporal_load(reinterpret_cast<const vfloat4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ inline void nt_store4(float* p, const float4& a) {
    vfloat4 v = {a.x, a.y, a.z, a.w};
    __builtin_nontemporal_store(v, reinterpret_cast<vfloat4*>(p));
}

__device__ inline void adam_update4(float4& p, const float4& g, float4& m, float4& v, const AdamShared& s,
                                    float bc2_sqrt, float neg_step) {
    adam_update(p.x, g.x, m.x, v.x, s.w1, s.beta2, s.w2, bc2_sqrt, s.eps, neg_step);
    adam_update(p.y, g.y, m.y, v.y, s.w1, s.beta2, s.w2, bc2_sqrt, s.eps, neg_step);
    adam_update(p.z, g.z, m.z, v.z, s.w1, s.beta2, s.w2, bc2_sqrt, s.eps, neg_step);
    adam_update(p.w, g.w, m.w, v.w, s.w1, s.beta2, s.w2, bc2_sqrt, s.eps, neg_step);
}

}  // namespace gs
