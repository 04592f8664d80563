// Inner optimizer on the flat arena: fused Adam/AdamW step and gradient-norm
// clipping, one streaming pass each instead of torch's ~10 multi-tensor passes
// (torch/optim/adam.py _multi_tensor_adam) behind the reference's
// `clip_grad_norm_` + `self.optim.step()` (strategy.py:135-140,
// communicate_optimize_strategy.py:69-73, diloco.py:52-59).  Roofline: HBM.
//
// Per element (f32 arena, f32 state), in torch's op order:
//   g  = grad * clip_coef                       (clip_grad_norm_, if clipping)
//   p *= 1 - lr*wd                              (AdamW: decoupled decay)   | g += wd*p (Adam: L2)
//   m  = lerp(m, g, 1-b1)                       (torch's lerp: m + w*(g-m) for w < 0.5)
//   v  = b2*v + (1-b2)*g*g
//   p += step_size * m / (sqrt(v)/bc2_sqrt + eps),  step_size = -lr/(1-b1^t), bc2_sqrt = sqrt(1-b2^t)
// 28 bytes per element (read p, g, m, v; write p, m, v), +4 when the clipped
// gradient is written back.
//
// SGD (torch.optim.SGD: momentum, dampening, Nesterov, L2 weight decay) is the same
// pass with fewer streams (sgd_math.h): 12 bytes per element without momentum (read
// p, g; write p), 20 with (the momentum buffer read and written), 16 on a parameter's
// first step (the buffer is only written), +4 when the clipped gradient is written back.
#include "ga_common.h"
#include "adam_math.h"
#include "sgd_math.h"


namespace ga {

constexpr int kOptBlock = 256;
constexpr int64_t kOptChunk = 1024;  // float4 vectors per workgroup
constexpr int kSumsqBlocks = 1024;   // partials of the norm reduction

// What one pass does per element.  An operation states at compile time its fp32 state
// streams (kStates), whether they are loaded (kLoad; they are always stored), whether
// the clip coefficient applies (kClip) and whether the n % 4 tail exists (kTail), and
// updates one element: operator()(p, g, s), s the element's kStates state values.
struct AdamOp {  // ga_adam_step: exp_avg, exp_avg_sq
    static constexpr int kStates = 2;
    static constexpr bool kLoad = true, kClip = true, kTail = true;
    AdamParams ap;
    __device__ __forceinline__ void operator()(float& p, float& g, float* s) const { adam_elem(p, g, s[0], s[1], ap); }
};

// ga_sgd_step.  kMomentum / kFirst / kNesterov are uniform over a launch; without
// momentum there is no state stream and the buffer pointer is never touched (it may be
// null), on a first step the buffer is written and not read.
template <bool kMomentum, bool kFirst, bool kNesterov>
struct SgdOp {
    static constexpr int kStates = kMomentum ? 1 : 0;
    static constexpr bool kLoad = !kFirst, kClip = true, kTail = true;
    SgdParams sp;
    __device__ __forceinline__ void operator()(float& p, float& g, float* s) const {
        sgd_elem<kMomentum, kFirst, kNesterov>(p, g, s[0], sp);
    }
};

// Placement probe of AdamOp (no reference counterpart): its exact access pattern (p, g,
// m, v read, p, m, v written through the same stores) with every value written back
// unchanged, so ArenaAdam can time candidate physical buffers for the moments without
// side effects.  No clip and no tail: ga_probe_adam_placement requires n % 4 == 0.
struct AdamProbeOp {
    static constexpr int kStates = 2;
    static constexpr bool kLoad = true, kClip = false, kTail = false;
    __device__ __forceinline__ void operator()(float&, float& g, float*) const {
        asm volatile("" ::"v"(g));  // the grad load stays live
    }
};

// The one streaming pass of the inner optimizers over [K, ld] sets: the replica
// (simulated node) on grid.y, kOptChunk float4 per workgroup, nt loads, the clipped
// gradient written back (clip_grad_norm_ leaves the clipped grads), sc1 stores, the
// scalar tail (n % 4) in the last workgroup.  s0 / s1 are the operation's state streams.
template <typename Op>
__global__ __launch_bounds__(kOptBlock) void opt_pass(float* __restrict__ param, float* __restrict__ grad,
                                                       float* __restrict__ s0, float* __restrict__ s1, int64_t n,
                                                       int64_t ld, Op op, const float* __restrict__ clip_coef) {
    constexpr int kS = Op::kStates, kSN = kS > 0 ? kS : 1;
    const int64_t rep = blockIdx.y;
    param += rep * ld;
    grad += rep * ld;
    float* st[2] = {s0, s1};
#pragma unroll
    for (int k = 0; k < kS; ++k) st[k] += rep * ld;
    float coef = 1.f;
    if constexpr (Op::kClip) coef = clip_coef ? clip_coef[2 * rep] : 1.f;
    const bool scale = !(coef >= 1.f);  // a NaN coefficient scales too (clamp(nan, max=1) is nan)
    const int64_t nv = n >> 2;
    const int64_t lo = (int64_t)blockIdx.x * kOptChunk;
    const int64_t hi = lo + kOptChunk < nv ? lo + kOptChunk : nv;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kOptBlock) {
        float pp[4], gg[4], ss[kSN][4] = {};
        Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(param) + i), pp);
        Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(grad) + i), gg);
#pragma unroll
        for (int k = 0; k < kS; ++k)
            if (Op::kLoad) Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(st[k]) + i), ss[k]);
        if (scale) {
#pragma unroll
            for (int e = 0; e < 4; ++e) gg[e] *= coef;
            stream_store(reinterpret_cast<float4*>(grad) + i, Vec4<float>::pack(gg));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s[kSN];
            for (int k = 0; k < kSN; ++k) s[k] = ss[k][e];
            op(pp[e], gg[e], s);
            for (int k = 0; k < kSN; ++k) ss[k][e] = s[k];
        }
        const uint32_t o = (uint32_t)(i - lo);
        store_sc1(reinterpret_cast<float4*>(param) + lo, o, Vec4<float>::pack(pp));
#pragma unroll
        for (int k = 0; k < kS; ++k) store_sc1(reinterpret_cast<float4*>(st[k]) + lo, o, Vec4<float>::pack(ss[k]));
    }
    if constexpr (Op::kTail) {
        if (blockIdx.x == gridDim.x - 1) {
            for (int64_t j = (nv << 2) + threadIdx.x; j < n; j += kOptBlock) {
                float p = param[j], g = grad[j], s[kSN] = {};
#pragma unroll
                for (int k = 0; k < kS; ++k)
                    if (Op::kLoad) s[k] = st[k][j];
                if (scale) {
                    g *= coef;
                    grad[j] = g;
                }
                op(p, g, s);
                param[j] = p;
#pragma unroll
                for (int k = 0; k < kS; ++k) st[k][j] = s[k];
            }
        }
    }
}

// partials[b] = sum of x^2 over a grid-stride share of the arena (fp32, fixed order)
template <typename T>
__global__ __launch_bounds__(kOptBlock) void sumsq_kernel(const T* __restrict__ x, int64_t n, int64_t ld,
                                                          float* __restrict__ partials) {
    __shared__ float red[kOptBlock / 64];
    x += (int64_t)blockIdx.y * ld;
    partials += (int64_t)blockIdx.y * gridDim.x;
    float acc = 0.f;
    const int64_t stride = (int64_t)gridDim.x * kOptBlock;
    const int64_t nv = ((uintptr_t)x % (4 * sizeof(T)) == 0) ? n / 4 : 0;  // 4-element vectors
    using V = typename Vec4<T>::type;
    for (int64_t i = (int64_t)blockIdx.x * kOptBlock + threadIdx.x; i < nv; i += stride) {
        float f[4];
        Vec4<T>::unpack(stream_load(reinterpret_cast<const V*>(x) + i), f);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(f[e], f[e], acc);
    }
    for (int64_t i = 4 * nv + (int64_t)blockIdx.x * kOptBlock + threadIdx.x; i < n; i += stride) {
        const float f = Elem<T>::load(x + i);
        acc = fmaf(f, f, acc);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = clamp(max_norm / (sqrt(sum partials) + 1e-6), max=1), out[1] = the total norm
// (torch.nn.utils.clip_grad_norm_ with norm_type 2; NaN norm -> NaN coefficient,
// infinite norm -> 0)
__global__ __launch_bounds__(kOptBlock) void clip_coef_kernel(const float* __restrict__ partials, int np,
                                                              float max_norm, float* __restrict__ out) {
    __shared__ float red[kOptBlock / 64];
    partials += (int64_t)blockIdx.x * np;  // one workgroup per replica
    out += 2 * (int64_t)blockIdx.x;
    float acc = 0.f;
    for (int i = threadIdx.x; i < np; i += kOptBlock) acc += partials[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float total = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
        const float c = max_norm / (total + 1e-6f);
        out[0] = c >= 1.f ? 1.f : c;  // torch's clamp(c, max=1): a NaN norm gives a NaN coefficient
        out[1] = total;
    }
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int ga_sumsq_partials_count(void) { return kSumsqBlocks; }

extern "C" GA_API int ga_grad_clip_coef(int dtype, const void* grad, int64_t K, int64_t ld, int64_t n,
                                        float max_norm, float* partials, float* out, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1 && K <= 65535, "ga_grad_clip_coef: bad sizes n=%lld K=%lld", (long long)n,
               (long long)K);
    GA_REQUIRE(K == 1 || ld >= n, "ga_grad_clip_coef: ld < n");
    GA_REQUIRE(grad && partials && out, "ga_grad_clip_coef: null buffer");
    GA_REQUIRE(max_norm > 0.f, "ga_grad_clip_coef: max_norm must be > 0");
    const int blocks = kSumsqBlocks;
    switch (dtype) {
        case GA_F32:
            hipLaunchKernelGGL(sumsq_kernel<float>, dim3(blocks, (unsigned)K), dim3(kOptBlock), 0, stream,
                               (const float*)grad, n, ld, partials);
            break;
        case GA_BF16:
            hipLaunchKernelGGL(sumsq_kernel<__hip_bfloat16>, dim3(blocks, (unsigned)K), dim3(kOptBlock), 0, stream,
                               (const __hip_bfloat16*)grad, n, ld, partials);
            break;
        default: set_error("ga_grad_clip_coef: unknown dtype %d", dtype); return GA_EINVAL;
    }
    if (int e = check_launch("ga_grad_clip_coef (sumsq)")) return e;
    hipLaunchKernelGGL(clip_coef_kernel, dim3((unsigned)K), dim3(kOptBlock), 0, stream, partials, blocks, max_norm,
                       out);
    return check_launch("ga_grad_clip_coef");
}

// What every pass requires of its sizes, in the entry point's name; *grid = workgroups
// per replica, 0 when there is nothing to do (n == 0).
static int opt_grid(const char* who, bool sizes_ok, int64_t n, int64_t K, int64_t ld, int64_t* grid) {
    *grid = 0;
    GA_REQUIRE(sizes_ok && n >= 0 && K >= 1 && K <= 65535, "%s: bad sizes n=%lld K=%lld", who, (long long)n,
               (long long)K);
    if (n == 0) return GA_OK;
    GA_REQUIRE(K == 1 || (ld >= n && ld % 4 == 0), "%s: ld must be >= n and a multiple of 4", who);
    const int64_t g = (n / 4 + kOptChunk - 1) / kOptChunk;
    *grid = g < 1 ? 1 : g;
    return GA_OK;
}

static bool aligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
    return ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) % 16 == 0;
}

template <typename Op>
static int opt_launch(const char* who, int64_t grid, int64_t K, hipStream_t stream, float* param, float* grad,
                      float* s0, float* s1, int64_t n, int64_t ld, Op op, const float* clip_coef) {
    hipLaunchKernelGGL(opt_pass<Op>, dim3((unsigned)grid, (unsigned)K), dim3(kOptBlock), 0, stream, param, grad, s0,
                       s1, n, ld, op, clip_coef);
    return check_launch(who);
}

extern "C" GA_API int ga_adam_step(int dtype, void* param, void* grad, float* exp_avg, float* exp_avg_sq, int64_t K,
                                   int64_t ld, int64_t n, float lerp_w, float beta2, float one_m_beta2, float eps,
                                   float wd_factor, float l2_wd, float step_size, float bc2_sqrt,
                                   const float* clip_coef, hipStream_t stream) {
    clear_error();
    int64_t grid;
    if (int e = opt_grid("ga_adam_step", true, n, K, ld, &grid)) return e;
    if (grid == 0) return GA_OK;
    GA_REQUIRE(param && grad && exp_avg && exp_avg_sq, "ga_adam_step: null buffer");
    GA_REQUIRE(dtype == GA_F32, "ga_adam_step: only float32 arenas are fused (dtype %d)", dtype);
    GA_REQUIRE(aligned16(param, grad, exp_avg, exp_avg_sq), "ga_adam_step: buffers must be 16-byte aligned");
    GA_REQUIRE(bc2_sqrt > 0.f, "ga_adam_step: bc2_sqrt must be > 0");
    const AdamOp op{{lerp_w, beta2, one_m_beta2, eps, wd_factor, l2_wd, step_size, bc2_sqrt}};
    return opt_launch("ga_adam_step", grid, K, stream, (float*)param, (float*)grad, exp_avg, exp_avg_sq, n, ld, op,
                      clip_coef);
}

extern "C" GA_API int ga_sgd_step(int dtype, void* param, void* grad, float* momentum_buf, int64_t K, int64_t ld,
                                  int64_t n, float neg_lr, float momentum, float one_m_dampening, float weight_decay,
                                  int nesterov, int first, const float* clip_coef, hipStream_t stream) {
    clear_error();
    int64_t grid;
    if (int e = opt_grid("ga_sgd_step", true, n, K, ld, &grid)) return e;
    if (grid == 0) return GA_OK;
    const bool mom = momentum != 0.f;
    GA_REQUIRE(param && grad, "ga_sgd_step: null buffer");
    GA_REQUIRE(!mom || momentum_buf, "ga_sgd_step: null momentum buffer with momentum %g", (double)momentum);
    GA_REQUIRE(dtype == GA_F32, "ga_sgd_step: only float32 arenas are fused (dtype %d)", dtype);
    GA_REQUIRE(aligned16(param, grad, mom ? momentum_buf : nullptr), "ga_sgd_step: buffers must be 16-byte aligned");
    const SgdParams sp{neg_lr, momentum, one_m_dampening, weight_decay};
#define GA_SGD_LAUNCH(M, F, N)                                                                                  \
    opt_launch("ga_sgd_step", grid, K, stream, (float*)param, (float*)grad, momentum_buf, nullptr, n, ld, \
               SgdOp<M, F, N>{sp}, clip_coef)
    if (!mom) return GA_SGD_LAUNCH(false, false, false);
    if (first) return nesterov ? GA_SGD_LAUNCH(true, true, true) : GA_SGD_LAUNCH(true, true, false);
    return nesterov ? GA_SGD_LAUNCH(true, false, true) : GA_SGD_LAUNCH(true, false, false);
#undef GA_SGD_LAUNCH
}

extern "C" GA_API int ga_probe_adam_placement(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                              int64_t K, int64_t ld, int64_t n, hipStream_t stream) {
    clear_error();
    int64_t grid;
    if (int e = opt_grid("ga_probe_adam_placement", n % 4 == 0, n, K, ld, &grid)) return e;
    if (grid == 0) return GA_OK;
    GA_REQUIRE(param && grad && exp_avg && exp_avg_sq, "ga_probe_adam_placement: null buffer");
    GA_REQUIRE(aligned16(param, grad, exp_avg, exp_avg_sq), "ga_probe_adam_placement: buffers must be 16-byte aligned");
    // the probe never writes the gradient (no clip)
    return opt_launch("ga_probe_adam_placement", grid, K, stream, param, const_cast<float*>(grad), exp_avg,
                      exp_avg_sq, n, ld, AdamProbeOp{}, nullptr);
}
