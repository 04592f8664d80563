// Replica mean-reduce and the fused DiLoCo outer step: HBM-streaming kernels
// over [K, ld] replica sets.  Roofline: HBM.
//
// Both kernels walk the arena in 4-element vectors (16 B per lane for f32,
// 8 B for bf16); workgroup b owns the contiguous vectors [b*kChunk,
// (b+1)*kChunk) (measured on MI355X: 5.1 TB/s for the K=8 DiLoCo stream vs
// 4.7 TB/s with a grid-stride loop; a plain float4 copy peaks at 5.2-5.5 TB/s
// on the same box, tools/ubench_stream.hip); every stream is loaded and stored
// non-temporally (stream_load / stream_store: 1.93 -> 1.88 ms for the K = 8 step
// on one box, profiles/r02z_ab_stream_nt.txt).  Each lane issues the K replica loads
// of one vector back to back (the k loop is unrolled so the loads are in
// flight together) and sums them in ascending k, so the result does not
// depend on the launch geometry.  dst may alias src (in-place average): each
// lane reads every replica of its vector before it writes any, and no two
// lanes touch the same vector, so the sources carry no __restrict__.
//
// The outer step exists three times: diloco_outer_kernel (SGD / Nesterov on the
// pseudo-gradient, ga_diloco_outer[_masked]), diloco_outer_adam_kernel (Adam /
// AdamW, ga_diloco_outer_adam[_masked]: one more fp32 state stream, adam_math.h's
// element update) and diloco_outer_merge_kernel (ga_diloco_outer_merge: the SGD step
// whose result is mixed into the live rows).  They share the geometry and the helpers
// below, the first two also the selectors.
#include "ga_common.h"
#include "adam_math.h"

namespace ga {

constexpr int kBlock = 256;
constexpr int64_t kChunk = 1024;  // vectors (or scalars) per workgroup

__device__ __forceinline__ void chunk_range(int64_t total, int64_t& lo, int64_t& hi) {
    lo = (int64_t)blockIdx.x * kChunk;
    hi = lo + kChunk < total ? lo + kChunk : total;
}

inline int chunk_grid(int64_t total) {
    const int64_t g = ceil_div(total, kChunk);
    return (int)(g < 1 ? 1 : g);
}

template <typename T>
__device__ __forceinline__ const T* replica_ptr(const T* base, const int32_t* rows, int64_t k,
                                                int64_t ld) {
    const int64_t r = rows ? (int64_t)rows[k] : k;
    return base + r * ld;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void replica_mean_kernel(
    const T* src, int64_t K, int64_t ld_src, const int32_t* __restrict__ rows,
    int64_t n, float divisor, T* dst, int64_t K_out, int64_t ld_dst) {
    const bool divide = divisor != 1.0f;
    int64_t lo, hi;
    if constexpr (VEC) {
        using V = typename Vec4<T>::type;
        chunk_range(n >> 2, lo, hi);
        for (int64_t v = lo + threadIdx.x; v < hi; v += kBlock) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int64_t k = 0; k < K; ++k) {
                const V raw = stream_load(reinterpret_cast<const V*>(replica_ptr(src, rows, k, ld_src)) + v);
                float f[4];
                Vec4<T>::unpack(raw, f);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += f[e];
            }
            if (divide) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = acc[e] / divisor;
            }
            const V out = Vec4<T>::pack(acc);
            for (int64_t j = 0; j < K_out; ++j) stream_store(reinterpret_cast<V*>(dst + j * ld_dst) + v, out);
        }
    } else {
        chunk_range(n, lo, hi);
        for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
            float acc = 0.f;
#pragma unroll 4
            for (int64_t k = 0; k < K; ++k) acc += Elem<T>::load(replica_ptr(src, rows, k, ld_src) + i);
            if (divide) acc = acc / divisor;
            for (int64_t j = 0; j < K_out; ++j) Elem<T>::store(dst + j * ld_dst + i, acc);
        }
    }
}

// One element of the DiLoCo outer update; mirrors torch.optim.SGD's
// single-tensor path (torch/optim/sgd.py) on the pseudo-gradient.
struct OuterParams {
    float divisor, lr, momentum, dampening, weight_decay;
    int first_step, nesterov;
};

__device__ __forceinline__ float outer_update(float sum, float& master, float& buf,
                                              const OuterParams& op) {
    const float avg = sum / op.divisor;
    float g = master - avg;
    if (op.weight_decay != 0.f) g = fmaf(op.weight_decay, master, g);
    if (op.momentum != 0.f) {
        if (op.first_step) buf = g;
        else buf = fmaf(1.f - op.dampening, g, buf * op.momentum);
        g = op.nesterov ? fmaf(op.momentum, buf, g) : buf;
    }
    master = fmaf(-op.lr, g, master);
    return master;
}

// The value an arena of dtype T holds after storing x (SPARTA writes its average
// to the replicas before the outer step reads them back).
template <typename T> __device__ __forceinline__ float round_to(float x);
template <> __device__ __forceinline__ float round_to<float>(float x) { return x; }
template <> __device__ __forceinline__ float round_to<__hip_bfloat16>(float x) {
    return __bfloat162float(__float2bfloat16(x));
}

// What the outer step sums over an element SPARTA averaged just before it: every
// replica then holds a = sum / sparse_divisor rounded to T, and the ascending
// fp32 sum of K copies of a is K additions (not K * a: the partial sums round).
template <typename T>
__device__ __forceinline__ float sum_of_sparse_average(float sum, float sparse_divisor, int64_t K) {
    const float a = round_to<T>(sum / sparse_divisor);
    float s = 0.f;
    for (int64_t k = 0; k < K; ++k) s += a;
    return s;
}

// Which elements of the outer step take sum_of_sparse_average instead of the plain
// replica sum.  DenseSel (ga_diloco_outer): none, and the kernel holds no mask code.
// SparseSel (ga_diloco_outer_masked, SPARTA's sparse average followed by the outer
// step in the outer step's one pass): those whose bit is set in `bits` (bit j of word
// w = element 64 w + j).  A lane's 4 elements are one nibble of a word, the 16 lanes
// of a word load the same 8 bytes; at SPARTA's rates the nibble is almost always 0
// and the selected branch is skipped.
struct DenseSel {};
struct SparseSel {
    const uint64_t* __restrict__ bits;
    float sparse_divisor;
    __device__ __forceinline__ uint32_t nibble(int64_t v) const {
        return (uint32_t)(bits[v >> 4] >> ((v & 15) * 4)) & 0xfu;
    }
    __device__ __forceinline__ bool bit(int64_t i) const { return bits[i >> 6] >> (i & 63) & 1ull; }
};

template <typename T, typename M, bool VEC, typename Sel>
__global__ __launch_bounds__(kBlock) void diloco_outer_kernel(
    const T* src, int64_t K, int64_t ld_src, int64_t n, M* master, M* mom,
    OuterParams op, T* dst, int64_t K_out, int64_t ld_dst, Sel sel) {
    constexpr bool kSparse = !std::is_same<Sel, DenseSel>::value;
    if constexpr (kSparse) {  // in place over all K rows, as ga_diloco_outer_masked requires: one K, one ld
        dst = const_cast<T*>(src);
        K_out = K;
        ld_dst = ld_src;
    }
    const bool has_mom = op.momentum != 0.f;
    int64_t lo, hi;
    if constexpr (VEC) {
        using V = typename Vec4<T>::type;
        using VM = typename Vec4<M>::type;
        chunk_range(n >> 2, lo, hi);
        for (int64_t v = lo + threadIdx.x; v < hi; v += kBlock) {
            uint32_t nib = 0;
            if constexpr (kSparse) nib = sel.nibble(v);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int64_t k = 0; k < K; ++k) {
                float f[4];
                Vec4<T>::unpack(stream_load(reinterpret_cast<const V*>(src + k * ld_src) + v), f);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += f[e];
            }
            if constexpr (kSparse) {
                if (nib) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (nib >> e & 1u) acc[e] = sum_of_sparse_average<T>(acc[e], sel.sparse_divisor, K);
                }
            }
            float m[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            Vec4<M>::unpack(stream_load(reinterpret_cast<const VM*>(master) + v), m);
            if (has_mom && !op.first_step) Vec4<M>::unpack(stream_load(reinterpret_cast<const VM*>(mom) + v), b);
            float out[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = outer_update(acc[e], m[e], b[e], op);
            const V o = Vec4<T>::pack(out);
            // device-scope (sc1) stores based at the workgroup's block of each stream
            const uint32_t i = (uint32_t)(v - lo);
            store_sc1(reinterpret_cast<VM*>(master) + lo, i, Vec4<M>::pack(m));
            if (has_mom) store_sc1(reinterpret_cast<VM*>(mom) + lo, i, Vec4<M>::pack(b));
            for (int64_t j = 0; j < K_out; ++j) store_sc1(reinterpret_cast<V*>(dst + j * ld_dst) + lo, i, o);
        }
    } else {
        chunk_range(n, lo, hi);
        for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
            float acc = 0.f;
#pragma unroll 4
            for (int64_t k = 0; k < K; ++k) acc += Elem<T>::load(src + k * ld_src + i);
            if constexpr (kSparse) {
                if (sel.bit(i)) acc = sum_of_sparse_average<T>(acc, sel.sparse_divisor, K);
            }
            float m = Elem<M>::load(master + i);
            float b = (has_mom && !op.first_step) ? Elem<M>::load(mom + i) : 0.f;
            const float out = outer_update(acc, m, b, op);
            Elem<M>::store(master + i, m);
            if (has_mom) Elem<M>::store(mom + i, b);
            for (int64_t j = 0; j < K_out; ++j) Elem<T>::store(dst + j * ld_dst + i, out);
        }
    }
}

// The outer step with an Adam/AdamW update (ga_diloco_outer_adam[_masked]): the
// geometry, loads, stores and selectors of diloco_outer_kernel, one more fp32 state
// stream, adam_elem (adam_math.h, the inner optimizer's element update) on the
// pseudo-gradient master - avg.  Master and both moments are fp32; zero moments with
// the bias corrections of t = 1 give torch's first step, so there is no first flag.
// A sibling rather than an update functor of diloco_outer_kernel, so that kernel's
// machine code stays what the headline measurement ran.
template <typename T, bool VEC, typename Sel>
__global__ __launch_bounds__(kBlock) void diloco_outer_adam_kernel(
    const T* src, int64_t K, int64_t ld_src, int64_t n, float divisor, float* master, float* exp_avg,
    float* exp_avg_sq, AdamParams ap, T* dst, int64_t K_out, int64_t ld_dst, Sel sel) {
    constexpr bool kSparse = !std::is_same<Sel, DenseSel>::value;
    if constexpr (kSparse) {  // in place over all K rows, as ga_diloco_outer_adam_masked requires
        dst = const_cast<T*>(src);
        K_out = K;
        ld_dst = ld_src;
    }
    int64_t lo, hi;
    if constexpr (VEC) {
        using V = typename Vec4<T>::type;
        chunk_range(n >> 2, lo, hi);
        for (int64_t v = lo + threadIdx.x; v < hi; v += kBlock) {
            uint32_t nib = 0;
            if constexpr (kSparse) nib = sel.nibble(v);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int64_t k = 0; k < K; ++k) {
                float f[4];
                Vec4<T>::unpack(stream_load(reinterpret_cast<const V*>(src + k * ld_src) + v), f);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += f[e];
            }
            if constexpr (kSparse) {
                if (nib) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (nib >> e & 1u) acc[e] = sum_of_sparse_average<T>(acc[e], sel.sparse_divisor, K);
                }
            }
            float p[4], m[4], s[4];
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(master) + v), p);
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(exp_avg) + v), m);
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(exp_avg_sq) + v), s);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float g = p[e] - acc[e] / divisor;
                adam_elem(p[e], g, m[e], s[e], ap);
            }
            const V o = Vec4<T>::pack(p);
            const uint32_t i = (uint32_t)(v - lo);
            store_sc1(reinterpret_cast<float4*>(master) + lo, i, Vec4<float>::pack(p));
            store_sc1(reinterpret_cast<float4*>(exp_avg) + lo, i, Vec4<float>::pack(m));
            store_sc1(reinterpret_cast<float4*>(exp_avg_sq) + lo, i, Vec4<float>::pack(s));
            for (int64_t j = 0; j < K_out; ++j) store_sc1(reinterpret_cast<V*>(dst + j * ld_dst) + lo, i, o);
        }
    } else {
        chunk_range(n, lo, hi);
        for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
            float acc = 0.f;
#pragma unroll 4
            for (int64_t k = 0; k < K; ++k) acc += Elem<T>::load(src + k * ld_src + i);
            if constexpr (kSparse) {
                if (sel.bit(i)) acc = sum_of_sparse_average<T>(acc, sel.sparse_divisor, K);
            }
            float p = master[i], m = exp_avg[i], s = exp_avg_sq[i];
            float g = p - acc / divisor;
            adam_elem(p, g, m, s, ap);
            master[i] = p;
            exp_avg[i] = m;
            exp_avg_sq[i] = s;
            for (int64_t j = 0; j < K_out; ++j) Elem<T>::store(dst + j * ld_dst + i, p);
        }
    }
}

// The delayed, mixed merge of the streaming outer step (ga_diloco_outer_merge): the
// SGD / Nesterov outer update of diloco_outer_kernel on a staged sum (or on the live
// rows themselves), then every live row x_j <- alpha x_j + (1 - alpha) master instead
// of master.  The geometry, loads, stores and outer_update of diloco_outer_kernel; fp32
// master and momentum.  With alpha != 0 a lane loads up to kMergeRows rows of x back to
// back (the first group together with master and momentum, before the lane's first
// store), blends and stores them, then the next group.  x may alias src (same base, ld
// and row count): every source of a vector is read before any of the vector's stores,
// and row j of x is read before it is written and never after.  A sibling rather than
// a template parameter of diloco_outer_kernel, so that kernel's machine code stays what
// the headline measurement ran.
constexpr int kMergeRows = 4;

template <typename T, bool VEC, bool MIX>
__global__ __launch_bounds__(kBlock) void diloco_outer_merge_kernel(
    const T* src, int64_t K, int64_t ld_src, int64_t n, float* master, float* mom, OuterParams op, float alpha,
    T* x, int64_t K_out, int64_t ld_x) {
    const bool has_mom = op.momentum != 0.f;
    constexpr bool mix = MIX;  // alpha != 0; the alpha == 0 instance holds no blend code and no x registers
    const float keep = 1.f - alpha;
    int64_t lo, hi;
    if constexpr (VEC) {
        using V = typename Vec4<T>::type;
        chunk_range(n >> 2, lo, hi);
        for (int64_t v = lo + threadIdx.x; v < hi; v += kBlock) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int64_t k = 0; k < K; ++k) {
                float f[4];
                Vec4<T>::unpack(stream_load(reinterpret_cast<const V*>(src + k * ld_src) + v), f);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += f[e];
            }
            float m[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(master) + v), m);
            if (has_mom && !op.first_step) Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(mom) + v), b);
            V xs[kMergeRows];
            if constexpr (mix) {
#pragma unroll
                for (int r = 0; r < kMergeRows; ++r)
                    if (r < K_out) xs[r] = stream_load(reinterpret_cast<const V*>(x + r * ld_x) + v);
            }
            float out[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = outer_update(acc[e], m[e], b[e], op);
            // device-scope (sc1) stores based at the workgroup's block of each stream
            const uint32_t i = (uint32_t)(v - lo);
            store_sc1(reinterpret_cast<float4*>(master) + lo, i, Vec4<float>::pack(m));
            if (has_mom) store_sc1(reinterpret_cast<float4*>(mom) + lo, i, Vec4<float>::pack(b));
            if constexpr (!mix) {
                const V o = Vec4<T>::pack(out);
                for (int64_t j = 0; j < K_out; ++j) store_sc1(reinterpret_cast<V*>(x + j * ld_x) + lo, i, o);
            } else {
                float part[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) part[e] = keep * out[e];
                for (int64_t j0 = 0; j0 < K_out; j0 += kMergeRows) {
                    if (j0 != 0) {
#pragma unroll
                        for (int r = 0; r < kMergeRows; ++r)
                            if (j0 + r < K_out) xs[r] = stream_load(reinterpret_cast<const V*>(x + (j0 + r) * ld_x) + v);
                    }
#pragma unroll
                    for (int r = 0; r < kMergeRows; ++r) {
                        if (j0 + r < K_out) {
                            float f[4];
                            Vec4<T>::unpack(xs[r], f);
#pragma unroll
                            for (int e = 0; e < 4; ++e) f[e] = fmaf(alpha, f[e], part[e]);
                            store_sc1(reinterpret_cast<V*>(x + (j0 + r) * ld_x) + lo, i, Vec4<T>::pack(f));
                        }
                    }
                }
            }
        }
    } else {
        chunk_range(n, lo, hi);
        for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
            float acc = 0.f;
#pragma unroll 4
            for (int64_t k = 0; k < K; ++k) acc += Elem<T>::load(src + k * ld_src + i);
            float m = master[i];
            float b = (has_mom && !op.first_step) ? mom[i] : 0.f;
            const float out = outer_update(acc, m, b, op);
            master[i] = m;
            if (has_mom) mom[i] = b;
            if constexpr (!mix) {
                for (int64_t j = 0; j < K_out; ++j) Elem<T>::store(x + j * ld_x + i, out);
            } else {
                const float part = keep * out;
                for (int64_t j = 0; j < K_out; ++j) {
                    T* p = x + j * ld_x + i;
                    Elem<T>::store(p, fmaf(alpha, Elem<T>::load(p), part));
                }
            }
        }
    }
}

// Placement probe of the fused outer step (no reference counterpart): the exact
// access pattern of diloco_outer_kernel<float, float, true, DenseSel> -- workgroup b's block
// of K replica streams, master and momentum read, the same blocks written through
// the same stores -- with every value written back unchanged, so a caller can time
// candidate master/momentum buffers against a live replica set without side
// effects.  K <= kProbeK (the replicas are held in registers to be written back).
constexpr int kProbeK = 16;
__global__ __launch_bounds__(kBlock) void diloco_probe_kernel(float* src, int64_t K, int64_t ld_src, int64_t n,
                                                              float* master, float* mom) {
    int64_t lo, hi;
    chunk_range(n >> 2, lo, hi);
    for (int64_t v = lo + threadIdx.x; v < hi; v += kBlock) {
        float4 x[kProbeK];
#pragma unroll
        for (int k = 0; k < kProbeK; ++k)
            if (k < K) x[k] = stream_load(reinterpret_cast<const float4*>(src + k * ld_src) + v);
        const float4 m = stream_load(reinterpret_cast<const float4*>(master) + v);
        const float4 b = stream_load(reinterpret_cast<const float4*>(mom) + v);
        const uint32_t i = (uint32_t)(v - lo);
        store_sc1(reinterpret_cast<float4*>(master) + lo, i, m);
        store_sc1(reinterpret_cast<float4*>(mom) + lo, i, b);
#pragma unroll
        for (int k = 0; k < kProbeK; ++k)
            if (k < K) store_sc1(reinterpret_cast<float4*>(src + k * ld_src) + lo, i, x[k]);
    }
}

// Placement probe of the in-place replica mean (no reference counterpart): the access
// pattern of replica_mean_kernel<float, true> with dst == src -- workgroup b's block of
// the K replica streams loaded, then stored back non-temporally -- with every value
// written back unchanged.  K <= kProbeK.
__global__ __launch_bounds__(kBlock) void mean_probe_kernel(float* src, int64_t K, int64_t ld_src, int64_t n) {
    int64_t lo, hi;
    chunk_range(n >> 2, lo, hi);
    for (int64_t v = lo + threadIdx.x; v < hi; v += kBlock) {
        float4 x[kProbeK];
#pragma unroll
        for (int k = 0; k < kProbeK; ++k)
            if (k < K) x[k] = stream_load(reinterpret_cast<const float4*>(src + k * ld_src) + v);
#pragma unroll
        for (int k = 0; k < kProbeK; ++k)
            if (k < K) stream_store(reinterpret_cast<float4*>(src + k * ld_src) + v, x[k]);
    }
}

static bool aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

template <typename T>
static int launch_replica_mean(const void* src, int64_t K, int64_t ld_src, const int32_t* rows,
                               int64_t n, float divisor, void* dst, int64_t K_out,
                               int64_t ld_dst, hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = (n % 4 == 0) && (ld_src % 4 == 0) && (ld_dst % 4 == 0) &&
                     aligned(src, vb) && aligned(dst, vb);
    if (vec) {
        hipLaunchKernelGGL((replica_mean_kernel<T, true>), dim3(chunk_grid(n / 4)),
                           dim3(kBlock), 0, stream, (const T*)src, K, ld_src, rows, n, divisor,
                           (T*)dst, K_out, ld_dst);
    } else {
        hipLaunchKernelGGL((replica_mean_kernel<T, false>), dim3(chunk_grid(n)),
                           dim3(kBlock), 0, stream, (const T*)src, K, ld_src, rows, n, divisor,
                           (T*)dst, K_out, ld_dst);
    }
    return check_launch("ga_replica_mean");
}

// The outer step's launch; who = the entry point (ga_diloco_outer_masked runs it in
// place over all K rows with a SparseSel).
template <typename T, typename M, typename Sel = DenseSel>
static int launch_diloco(const char* who, const void* src, int64_t K, int64_t ld_src, int64_t n, void* master,
                         void* mom, const OuterParams& op, void* dst, int64_t K_out, int64_t ld_dst,
                         hipStream_t stream, Sel sel = Sel{}) {
    const int vb = 4 * (int)sizeof(T);
    const int vm = 4 * (int)sizeof(M);
    const bool vec = (n % 4 == 0) && (ld_src % 4 == 0) && (ld_dst % 4 == 0) &&
                     aligned(src, vb) && aligned(dst, vb) && aligned(master, vm) &&
                     aligned(mom, vm);
    if (vec) {
        hipLaunchKernelGGL((diloco_outer_kernel<T, M, true, Sel>), dim3(chunk_grid(n / 4)),
                           dim3(kBlock), 0, stream, (const T*)src, K, ld_src, n, (M*)master,
                           (M*)mom, op, (T*)dst, K_out, ld_dst, sel);
    } else {
        hipLaunchKernelGGL((diloco_outer_kernel<T, M, false, Sel>), dim3(chunk_grid(n)),
                           dim3(kBlock), 0, stream, (const T*)src, K, ld_src, n, (M*)master,
                           (M*)mom, op, (T*)dst, K_out, ld_dst, sel);
    }
    return check_launch(who);
}

// The Adam outer step's launch; state is fp32 whatever the arena's dtype.
template <typename T, typename Sel = DenseSel>
static int launch_diloco_adam(const char* who, const void* src, int64_t K, int64_t ld_src, int64_t n, float divisor,
                              float* master, float* exp_avg, float* exp_avg_sq, const AdamParams& ap, void* dst,
                              int64_t K_out, int64_t ld_dst, hipStream_t stream, Sel sel = Sel{}) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = (n % 4 == 0) && (ld_src % 4 == 0) && (ld_dst % 4 == 0) && aligned(src, vb) &&
                     aligned(dst, vb) && aligned(master, 16) && aligned(exp_avg, 16) && aligned(exp_avg_sq, 16);
    if (vec) {
        hipLaunchKernelGGL((diloco_outer_adam_kernel<T, true, Sel>), dim3(chunk_grid(n / 4)), dim3(kBlock), 0,
                           stream, (const T*)src, K, ld_src, n, divisor, master, exp_avg, exp_avg_sq, ap, (T*)dst,
                           K_out, ld_dst, sel);
    } else {
        hipLaunchKernelGGL((diloco_outer_adam_kernel<T, false, Sel>), dim3(chunk_grid(n)), dim3(kBlock), 0, stream,
                           (const T*)src, K, ld_src, n, divisor, master, exp_avg, exp_avg_sq, ap, (T*)dst, K_out,
                           ld_dst, sel);
    }
    return check_launch(who);
}

// The merge step's launch; the vector path by launch_diloco's rule.
template <typename T>
static int launch_diloco_merge(const void* src, int64_t K, int64_t ld_src, int64_t n, float* master, float* mom,
                               const OuterParams& op, float alpha, void* x, int64_t K_out, int64_t ld_x,
                               hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = (n % 4 == 0) && (ld_src % 4 == 0) && (ld_x % 4 == 0) && aligned(src, vb) && aligned(x, vb) &&
                     aligned(master, 16) && aligned(mom, 16);
    auto* kernel = vec ? (alpha != 0.f ? diloco_outer_merge_kernel<T, true, true> : diloco_outer_merge_kernel<T, true, false>)
                       : (alpha != 0.f ? diloco_outer_merge_kernel<T, false, true>
                                       : diloco_outer_merge_kernel<T, false, false>);
    hipLaunchKernelGGL(kernel, dim3(chunk_grid(vec ? n / 4 : n)), dim3(kBlock), 0, stream, (const T*)src, K, ld_src,
                       n, master, mom, op, alpha, (T*)x, K_out, ld_x);
    return check_launch("ga_diloco_outer_merge");
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int ga_replica_mean(int dtype, const void* src, int64_t K, int64_t ld_src,
                                      const int32_t* rows, int64_t n, float divisor, void* dst,
                                      int64_t K_out, int64_t ld_dst, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1 && K_out >= 0, "ga_replica_mean: bad sizes n=%lld K=%lld K_out=%lld",
               (long long)n, (long long)K, (long long)K_out);
    if (n == 0 || K_out == 0) return GA_OK;
    GA_REQUIRE(src && dst, "ga_replica_mean: null buffer");
    GA_REQUIRE(K == 1 || rows || ld_src >= n, "ga_replica_mean: ld_src %lld < n %lld", (long long)ld_src,
               (long long)n);
    GA_REQUIRE(K_out == 1 || ld_dst >= n, "ga_replica_mean: ld_dst %lld < n %lld", (long long)ld_dst,
               (long long)n);
    GA_REQUIRE(divisor != 0.0f, "ga_replica_mean: divisor is 0");
    switch (dtype) {
        case GA_F32:
            return launch_replica_mean<float>(src, K, ld_src, rows, n, divisor, dst, K_out, ld_dst, stream);
        case GA_BF16:
            return launch_replica_mean<__hip_bfloat16>(src, K, ld_src, rows, n, divisor, dst, K_out,
                                                       ld_dst, stream);
        default:
            set_error("ga_replica_mean: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer(int dtype, const void* src, int64_t K, int64_t ld_src,
                                      int64_t n, float divisor, void* master, void* mom,
                                      int master_f32, int first_step, float lr, float momentum,
                                      float dampening, float weight_decay, int nesterov,
                                      void* dst, int64_t K_out, int64_t ld_dst,
                                      hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1 && K_out >= 0, "ga_diloco_outer: bad sizes n=%lld K=%lld K_out=%lld",
               (long long)n, (long long)K, (long long)K_out);
    if (n == 0) return GA_OK;
    GA_REQUIRE(src && master, "ga_diloco_outer: null src/master");
    GA_REQUIRE(K_out == 0 || dst, "ga_diloco_outer: null dst");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(K == 1 || ld_src >= n, "ga_diloco_outer: ld_src < n");
    GA_REQUIRE(K_out <= 1 || ld_dst >= n, "ga_diloco_outer: ld_dst < n");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer: divisor is 0");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer: Nesterov momentum requires a momentum and zero dampening");
    OuterParams op{divisor, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    switch (dtype) {
        case GA_F32:
            return launch_diloco<float, float>("ga_diloco_outer", src, K, ld_src, n, master, mom, op, dst, K_out,
                                               ld_dst, stream);
        case GA_BF16:
            if (master_f32)
                return launch_diloco<__hip_bfloat16, float>("ga_diloco_outer", src, K, ld_src, n, master, mom, op,
                                                            dst, K_out, ld_dst, stream);
            return launch_diloco<__hip_bfloat16, __hip_bfloat16>("ga_diloco_outer", src, K, ld_src, n, master, mom,
                                                                 op, dst, K_out, ld_dst, stream);
        default:
            set_error("ga_diloco_outer: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_masked(int dtype, void* src, int64_t K, int64_t ld_src, int64_t n,
                                             const uint64_t* bits, float sparse_divisor, float divisor,
                                             void* master, void* mom, int master_f32, int first_step,
                                             float lr, float momentum, float dampening, float weight_decay,
                                             int nesterov, void* dst, int64_t K_out, int64_t ld_dst,
                                             hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_diloco_outer_masked: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    // the sparse average only vanishes into the outer step when that overwrites every row it wrote
    GA_REQUIRE(dst == src && K_out == K && (K == 1 || ld_dst == ld_src),
               "ga_diloco_outer_masked: the step must run in place over all K rows (dst == src, K_out == K = %lld, "
               "ld_dst == ld_src); got K_out=%lld", (long long)K, (long long)K_out);
    GA_REQUIRE(sparse_divisor > 0.0f, "ga_diloco_outer_masked: sparse_divisor must be > 0");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_masked: divisor is 0");
    if (n == 0) return GA_OK;
    GA_REQUIRE(bits != nullptr, "ga_diloco_outer_masked: null mask words");
    GA_REQUIRE(src && master, "ga_diloco_outer_masked: null src/master");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_masked: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(K == 1 || ld_src >= n, "ga_diloco_outer_masked: ld_src < n");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_masked: Nesterov momentum requires a momentum and zero dampening");
    GA_REQUIRE(dtype == GA_F32 || master_f32, "ga_diloco_outer_masked: master and momentum must be fp32");
    OuterParams op{divisor, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    const SparseSel sel{bits, sparse_divisor};
    const char* who = "ga_diloco_outer_masked";
    switch (dtype) {
        case GA_F32:
            return launch_diloco<float, float>(who, src, K, ld_src, n, master, mom, op, src, K, ld_src, stream, sel);
        case GA_BF16:
            return launch_diloco<__hip_bfloat16, float>(who, src, K, ld_src, n, master, mom, op, src, K, ld_src,
                                                        stream, sel);
        default:
            set_error("ga_diloco_outer_masked: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_merge(int dtype, const void* src, int64_t K, int64_t ld_src, int64_t n,
                                            float divisor, float* master, float* mom, int first_step, float lr,
                                            float momentum, float dampening, float weight_decay, int nesterov,
                                            float alpha, void* x, int64_t K_out, int64_t ld_x, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1 && K_out >= 0, "ga_diloco_outer_merge: bad sizes n=%lld K=%lld K_out=%lld",
               (long long)n, (long long)K, (long long)K_out);
    GA_REQUIRE(alpha >= 0.0f && alpha < 1.0f, "ga_diloco_outer_merge: alpha %g is not in [0, 1)", (double)alpha);
    if (n == 0) return GA_OK;
    GA_REQUIRE(src && master, "ga_diloco_outer_merge: null src/master");
    GA_REQUIRE(K_out == 0 || x, "ga_diloco_outer_merge: null x");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_merge: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(K == 1 || ld_src >= n, "ga_diloco_outer_merge: ld_src < n");
    GA_REQUIRE(K_out <= 1 || ld_x >= n, "ga_diloco_outer_merge: ld_x < n");
    GA_REQUIRE(x != src || K_out == 0 || (K_out == K && (K == 1 || ld_x == ld_src)),
               "ga_diloco_outer_merge: x aliasing src needs K_out == K = %lld and ld_x == ld_src; got K_out=%lld",
               (long long)K, (long long)K_out);
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_merge: divisor is 0");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_merge: Nesterov momentum requires a momentum and zero dampening");
    OuterParams op{divisor, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    switch (dtype) {
        case GA_F32:
            return launch_diloco_merge<float>(src, K, ld_src, n, master, mom, op, alpha, x, K_out, ld_x, stream);
        case GA_BF16:
            return launch_diloco_merge<__hip_bfloat16>(src, K, ld_src, n, master, mom, op, alpha, x, K_out, ld_x,
                                                       stream);
        default:
            set_error("ga_diloco_outer_merge: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_adam(int dtype, const void* src, int64_t K, int64_t ld_src, int64_t n,
                                           float divisor, float* master, float* exp_avg, float* exp_avg_sq,
                                           float lerp_w, float beta2, float one_m_beta2, float eps, float wd_factor,
                                           float l2_wd, float step_size, float bc2_sqrt, void* dst, int64_t K_out,
                                           int64_t ld_dst, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1 && K_out >= 0, "ga_diloco_outer_adam: bad sizes n=%lld K=%lld K_out=%lld",
               (long long)n, (long long)K, (long long)K_out);
    if (n == 0) return GA_OK;
    GA_REQUIRE(src && master, "ga_diloco_outer_adam: null src/master");
    GA_REQUIRE(exp_avg && exp_avg_sq, "ga_diloco_outer_adam: null exp_avg/exp_avg_sq");
    GA_REQUIRE(K_out == 0 || dst, "ga_diloco_outer_adam: null dst");
    GA_REQUIRE(K == 1 || ld_src >= n, "ga_diloco_outer_adam: ld_src < n");
    GA_REQUIRE(K_out <= 1 || ld_dst >= n, "ga_diloco_outer_adam: ld_dst < n");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_adam: divisor is 0");
    const AdamParams ap{lerp_w, beta2, one_m_beta2, eps, wd_factor, l2_wd, step_size, bc2_sqrt};
    const char* who = "ga_diloco_outer_adam";
    switch (dtype) {
        case GA_F32:
            return launch_diloco_adam<float>(who, src, K, ld_src, n, divisor, master, exp_avg, exp_avg_sq, ap, dst,
                                             K_out, ld_dst, stream);
        case GA_BF16:
            return launch_diloco_adam<__hip_bfloat16>(who, src, K, ld_src, n, divisor, master, exp_avg, exp_avg_sq,
                                                      ap, dst, K_out, ld_dst, stream);
        default:
            set_error("ga_diloco_outer_adam: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_adam_masked(int dtype, void* src, int64_t K, int64_t ld_src, int64_t n,
                                                  const uint64_t* bits, float sparse_divisor, float divisor,
                                                  float* master, float* exp_avg, float* exp_avg_sq, float lerp_w,
                                                  float beta2, float one_m_beta2, float eps, float wd_factor,
                                                  float l2_wd, float step_size, float bc2_sqrt, void* dst,
                                                  int64_t K_out, int64_t ld_dst, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_diloco_outer_adam_masked: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    // the sparse average only vanishes into the outer step when that overwrites every row it wrote
    GA_REQUIRE(dst == src && K_out == K && (K == 1 || ld_dst == ld_src),
               "ga_diloco_outer_adam_masked: the step must run in place over all K rows (dst == src, K_out == K = "
               "%lld, ld_dst == ld_src); got K_out=%lld", (long long)K, (long long)K_out);
    GA_REQUIRE(sparse_divisor > 0.0f, "ga_diloco_outer_adam_masked: sparse_divisor must be > 0");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_adam_masked: divisor is 0");
    if (n == 0) return GA_OK;
    GA_REQUIRE(bits != nullptr, "ga_diloco_outer_adam_masked: null mask words");
    GA_REQUIRE(src && master, "ga_diloco_outer_adam_masked: null src/master");
    GA_REQUIRE(exp_avg && exp_avg_sq, "ga_diloco_outer_adam_masked: null exp_avg/exp_avg_sq");
    GA_REQUIRE(K == 1 || ld_src >= n, "ga_diloco_outer_adam_masked: ld_src < n");
    const AdamParams ap{lerp_w, beta2, one_m_beta2, eps, wd_factor, l2_wd, step_size, bc2_sqrt};
    const SparseSel sel{bits, sparse_divisor};
    const char* who = "ga_diloco_outer_adam_masked";
    switch (dtype) {
        case GA_F32:
            return launch_diloco_adam<float>(who, src, K, ld_src, n, divisor, master, exp_avg, exp_avg_sq, ap, src,
                                             K, ld_src, stream, sel);
        case GA_BF16:
            return launch_diloco_adam<__hip_bfloat16>(who, src, K, ld_src, n, divisor, master, exp_avg, exp_avg_sq,
                                                      ap, src, K, ld_src, stream, sel);
        default:
            set_error("ga_diloco_outer_adam_masked: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_probe_diloco_placement(float* src, int64_t K, int64_t ld_src, int64_t n, float* master,
                                                float* mom, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && n % 4 == 0 && K >= 1 && K <= kProbeK, "ga_probe_diloco_placement: bad sizes n=%lld K=%lld "
               "(n a multiple of 4, K <= %d)", (long long)n, (long long)K, kProbeK);
    if (n == 0) return GA_OK;
    GA_REQUIRE(src && master && mom, "ga_probe_diloco_placement: null buffer");
    GA_REQUIRE(K == 1 || (ld_src >= n && ld_src % 4 == 0), "ga_probe_diloco_placement: bad ld_src");
    GA_REQUIRE(aligned(src, 16) && aligned(master, 16) && aligned(mom, 16), "ga_probe_diloco_placement: alignment");
    hipLaunchKernelGGL(diloco_probe_kernel, dim3(chunk_grid(n / 4)), dim3(kBlock), 0, stream, src, K, ld_src, n,
                       master, mom);
    return check_launch("ga_probe_diloco_placement");
}

extern "C" GA_API int ga_probe_mean_placement(float* src, int64_t K, int64_t ld_src, int64_t n, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && n % 4 == 0 && K >= 1 && K <= kProbeK, "ga_probe_mean_placement: bad sizes n=%lld K=%lld "
               "(n a multiple of 4, K <= %d)", (long long)n, (long long)K, kProbeK);
    if (n == 0) return GA_OK;
    GA_REQUIRE(src != nullptr, "ga_probe_mean_placement: null buffer");
    GA_REQUIRE(K == 1 || (ld_src >= n && ld_src % 4 == 0), "ga_probe_mean_placement: bad ld_src");
    GA_REQUIRE(aligned(src, 16), "ga_probe_mean_placement: alignment");
    hipLaunchKernelGGL(mean_probe_kernel, dim3(chunk_grid(n / 4)), dim3(kBlock), 0, stream, src, K, ld_src, n);
    return check_launch("ga_probe_mean_placement");
}
