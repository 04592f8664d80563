// Arithmetic shared by the compressed outer steps (quant.hip, mx.hip): single rounded
// fp32 operations and ga_diloco_outer's element update from the pseudo-gradient on.
#pragma once

#include "ga_common.h"

namespace ga {

// One correctly rounded fp32 operation that no neighbour can be fused into.  hipcc
// contracts a * b + c across statements by default (-ffp-contract=fast-honor-pragmas),
// and its __fadd_rn / __fmul_rn are the plain operators under that default, so each
// operation is built here with contraction off.
__device__ __forceinline__ float rn_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float rn_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float rn_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float rn_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}

// ga_diloco_outer's element update from the pseudo-gradient on (reduce.hip, outer_update
// after `g = master - avg`); kept apart from that file so its machine code stays as measured.
struct QuantOuterParams {
    float divisor, lr, momentum, dampening, weight_decay;
    int first_step, nesterov;
};

// The update from the pseudo-gradient g itself (lowrank.hip forms g without a division).
__device__ __forceinline__ float outer_update_from_g(float g, float& master, float& buf,
                                                     const QuantOuterParams& op) {
    if (op.weight_decay != 0.f) g = fmaf(op.weight_decay, master, g);
    if (op.momentum != 0.f) {
        if (op.first_step) buf = g;
        else buf = fmaf(rn_sub(1.f, op.dampening), g, rn_mul(buf, op.momentum));
        g = op.nesterov ? fmaf(op.momentum, buf, g) : buf;
    }
    master = fmaf(-op.lr, g, master);
    return master;
}

__device__ __forceinline__ float quant_outer_update(float acc, float& master, float& buf,
                                                    const QuantOuterParams& op) {
    return outer_update_from_g(rn_div(acc, op.divisor), master, buf, op);
}

}  // namespace ga
