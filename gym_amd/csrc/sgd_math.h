// SGD element update of the inner-optimizer kernel (optim.hip).  Per element
// (f32 arena, f32 momentum buffer), in torch's op order (torch/optim/sgd.py,
// _single_tensor_sgd / _multi_tensor_sgd, the same sequence):
//   g   = g + wd*p                              (weight_decay != 0; the stored gradient keeps its value)
//   buf = g                                     (the parameter's first step: clone(grad), no dampening)
//       | momentum*buf + (1-dampening)*g        (later steps)
//   g   = g + momentum*buf (nesterov) | buf
//   p  += -lr * g
// The flags are compile-time, so a launch carries no per-element branch.
#pragma once

namespace ga {

struct SgdParams {
    float neg_lr, momentum, one_m_dampening, weight_decay;
};

template <bool kMomentum, bool kFirst, bool kNesterov>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, const SgdParams& sp) {
    if (sp.weight_decay != 0.f) g = fmaf(sp.weight_decay, p, g);  // uniform over the launch
    if (kMomentum) {
        buf = kFirst ? g : fmaf(sp.one_m_dampening, g, buf * sp.momentum);
        g = kNesterov ? fmaf(sp.momentum, buf, g) : buf;
    }
    p = fmaf(sp.neg_lr, g, p);
}

}  // namespace ga
