// Node-drift statistics of a [K, ld] replica set in one read: the K x K Gram
// matrix on the f32 MFMA, and the row sums and squared distances to the node mean
// on the VALU (replaces the reference's disabled model-correlation metric,
// exogym/train_node.py:498-573).  Roofline: HBM.
//
// A wavefront owns kWaveCols consecutive elements of every row and walks them in
// tiles of kTileCols.  A tile is loaded as in ga_replica_mean: lane c holds the
// 4-element vector at column 4c of each of the K rows (one coalesced 1-KiB segment
// per row and instruction), so the sum over the nodes of one element -- the node
// mean m[e] of dist2 -- is an ascending-k sum inside a lane, and rowsum / dist2 are
// per-lane accumulators.  The tile then goes through a wave-private LDS image
// [row][column] and comes back with the row on the lane, which is the MFMA's
// operand layout: lane l holds an element of row l & 31 (l & 15), lanes of equal
// l >> 5 (l >> 4) the same element index, and for a Gram matrix B = A^T, so the A
// register is the B operand too.  Rows >= K of the image stay zero.  The next
// tile's loads are issued before the MFMA loop of the current one.
//
// Determinism and precision: no atomics.  No fp32 accumulator takes more than
// kWaveCols multiply-adds (the MFMA is a k-ordered fmaf chain); the four waves'
// results are added in wave order and written as the workgroup's fp32 partial
// (K*K + 2K values), and gram_final_kernel sums the partials in a fixed order in fp64.
//
// ga_replica_gram_centered (CEN) is the same walk over d_k = x_k - m instead of x_k:
// the lane completes the node mean of its four columns before any row of the tile
// goes to LDS, and writes f - m.  The Gram matrix of the centred values keeps the
// pairwise distances and 1 - correlation of nodes that are 1e-3 and less apart,
// which G_ii + G_jj - 2 G_ij and G_ij - s_i s_j / n from the plain Gram matrix cancel
// away.  sum d_k and m . d_k take the registers of rowsum and dist2; sum m^2 and
// sum m are two more per-lane accumulators (partial: K*K + 2K + 2 values).
#include "ga_common.h"

namespace ga {

constexpr int kGramBlock = 256;
constexpr int kGramWaves = kGramBlock / 64;
constexpr int kTileCols = 256;                          // 64 lanes x one 4-element vector
constexpr int kTilesPerWave = 16;
constexpr int kWaveCols = kTileCols * kTilesPerWave;    // 4096: the fp32 chain bound
constexpr int kWgCols = kWaveCols * kGramWaves;         // 16384 columns per workgroup
constexpr int kStride = kTileCols + 4;                  // LDS row stride (floats), 16-B aligned rows
constexpr int kGramMaxK = 32;

typedef float ga_f16v __attribute__((ext_vector_type(16)));

static_assert(kWaveCols <= 4096, "chain bound of ga_replica_gram_chain()");

inline int64_t gram_grid(int64_t n) { return n <= 0 ? 0 : ceil_div(n, kWgCols); }
inline int64_t gram_partial_len(int64_t K) { return K * K + 2 * K; }
inline int64_t gram_centered_partial_len(int64_t K) { return K * K + 2 * K + 2; }

// Columns [col, col + 4) of one row, still in the arena's format (bf16 is widened where
// the values are used, so the loads stay in flight until then); columns >= n are never
// read and give 0.
template <bool VEC>
__device__ __forceinline__ float4 load_cols(const float* row, int64_t col, int64_t n) {
    if (VEC && col + 4 <= n) return stream_load(reinterpret_cast<const float4*>(row + col));
    float f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (col + e < n) f[e] = __builtin_nontemporal_load(row + col + e);
    return make_float4(f[0], f[1], f[2], f[3]);
}
template <bool VEC>
__device__ __forceinline__ uint2 load_cols(const __hip_bfloat16* row, int64_t col, int64_t n) {
    if (VEC && col + 4 <= n) return stream_load(reinterpret_cast<const uint2*>(row + col));
    uint32_t b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (col + e < n) b[e] = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(row + col + e));
    return make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
}

__device__ __forceinline__ void wave_lds_sync() {
    // the image is private to the wave: its LDS operations complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// KP = 32: v_mfma_f32_32x32x2_f32, KP = 16: v_mfma_f32_16x16x4_f32 (K <= KP).
// CEN: the centred form; rs[] then holds sum d_k, d2[] holds m . d_k, want_dist is unused.
template <typename T, int KP, bool VEC, bool CEN>
__global__ __launch_bounds__(kGramBlock) void gram_partial_kernel(const T* __restrict__ src, int K, int64_t ld,
                                                                  int64_t n, int want_dist,
                                                                  float* __restrict__ work) {
    __shared__ __attribute__((aligned(16))) float image[kGramWaves][KP * kStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* my = image[wave];
    for (int k = K; k < KP; ++k)
        *reinterpret_cast<float4*>(my + k * kStride + 4 * lane) = make_float4(0.f, 0.f, 0.f, 0.f);

    const int64_t col0 = (int64_t)blockIdx.x * kWgCols + (int64_t)wave * kWaveCols;
    const float fK = (float)K;
    using V = typename Vec4<T>::type;
    V x[KP];
    float rs[KP], d2[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        x[k] = V{};
        rs[k] = 0.f;
        d2[k] = 0.f;
    }
    float mm = 0.f, ms = 0.f;  // CEN: sum m^2, sum m
    ga_f16v acc32 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    ga_f4 acc16a = {0.f, 0.f, 0.f, 0.f}, acc16b = {0.f, 0.f, 0.f, 0.f};

    if (col0 < n) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) x[k] = load_cols<VEC>(src + (int64_t)k * ld, col0 + 4 * lane, n);
    }
    for (int t = 0; t < kTilesPerWave; ++t) {
        const int64_t c0 = col0 + (int64_t)t * kTileCols;
        if (c0 >= n) break;  // wave-uniform
        // node mean of the lane's four elements: fp32 sum in ascending k, true division
        float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (k < K) {
                float f[4];
                Vec4<T>::unpack(x[k], f);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    m[e] += f[e];
                    if constexpr (!CEN) rs[k] += f[e];
                }
                if constexpr (!CEN)
                    *reinterpret_cast<float4*>(my + k * kStride + 4 * lane) = make_float4(f[0], f[1], f[2], f[3]);
            }
        }
        if (CEN || want_dist) {
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = m[e] / fK;
            if constexpr (CEN) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    mm = fmaf(m[e], m[e], mm);
                    ms += m[e];
                }
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                if (k < K) {
                    float f[4];
                    Vec4<T>::unpack(x[k], f);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float q = f[e] - m[e];
                        if constexpr (CEN) {
                            // the mean is complete: the image takes f - m (0 at columns >= n,
                            // where every row reads as 0)
                            f[e] = q;
                            rs[k] += q;
                            d2[k] = fmaf(m[e], q, d2[k]);
                        } else {
                            d2[k] = fmaf(q, q, d2[k]);
                        }
                    }
                    if constexpr (CEN)
                        *reinterpret_cast<float4*>(my + k * kStride + 4 * lane) = make_float4(f[0], f[1], f[2], f[3]);
                }
            }
        }
        wave_lds_sync();
        // the next tile's loads fly during this tile's MFMA loop
        if (t + 1 < kTilesPerWave && c0 + kTileCols < n) {
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K) x[k] = load_cols<VEC>(src + (int64_t)k * ld, c0 + kTileCols + 4 * lane, n);
        }
        if constexpr (KP == 32) {
            // lane (r = l & 31, h = l >> 5): columns 8j + 4h + e; MFMA e of step j sums the
            // two columns 8j + e and 8j + 4 + e
            const float* rd = my + (lane & 31) * kStride + 4 * (lane >> 5);
#pragma unroll 4
            for (int j = 0; j < kTileCols / 8; ++j) {
                const float4 a = *reinterpret_cast<const float4*>(rd + 8 * j);
                acc32 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, a.x, acc32, 0, 0, 0);
                acc32 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, a.y, acc32, 0, 0, 0);
                acc32 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, a.z, acc32, 0, 0, 0);
                acc32 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, a.w, acc32, 0, 0, 0);
            }
        } else {
            // lane (r = l & 15, g = l >> 4): columns 16j + 4g + e; two accumulators cover the
            // instruction's dependent latency, each takes half of the wave's columns
            const float* rd = my + (lane & 15) * kStride + 4 * (lane >> 4);
#pragma unroll 4
            for (int j = 0; j < kTileCols / 16; ++j) {
                const float4 a = *reinterpret_cast<const float4*>(rd + 16 * j);
                acc16a = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, a.x, acc16a, 0, 0, 0);
                acc16b = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, a.y, acc16b, 0, 0, 0);
                acc16a = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, a.z, acc16a, 0, 0, 0);
                acc16b = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, a.w, acc16b, 0, 0, 0);
            }
        }
        wave_lds_sync();
    }

    // the wave's results into its own image: [KP x KP] Gram, rowsum, dist2 (CEN: sum d, m . d, then sum m^2, sum m)
    float* out = my;
    if constexpr (KP == 32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            out[row * KP + (lane & 31)] = acc32[r];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[((lane >> 4) * 4 + r) * KP + (lane & 15)] = acc16a[r] + acc16b[r];
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (k < K) {
            const float s = wave_sum(rs[k]);
            const float d = (CEN || want_dist) ? wave_sum(d2[k]) : 0.f;
            if (lane == 0) {
                out[KP * KP + k] = s;
                out[KP * KP + KP + k] = d;
            }
        }
    }
    constexpr int kExtra = CEN ? 2 : 0;
    if constexpr (CEN) {
        mm = wave_sum(mm);
        ms = wave_sum(ms);
        if (lane == 0) {
            out[KP * KP + 2 * KP] = mm;
            out[KP * KP + 2 * KP + 1] = ms;
        }
    }
    __syncthreads();
    float* part = work + (int64_t)blockIdx.x * (K * K + 2 * K + kExtra);
    for (int i = threadIdx.x; i < KP * KP + 2 * KP + kExtra; i += kGramBlock) {
        float v = image[0][i];
#pragma unroll
        for (int w = 1; w < kGramWaves; ++w) v += image[w][i];
        if (i < KP * KP) {
            const int row = i / KP, col = i % KP;
            if (row < K && col < K) part[row * K + col] = v;
        } else if (i < KP * KP + 2 * KP) {
            const int which = (i - KP * KP) / KP, k = (i - KP * KP) % KP;
            if (k < K) part[K * K + which * K + k] = v;
        } else {
            part[K * K + 2 * K + (i - KP * KP - 2 * KP)] = v;
        }
    }
}

// out[e] = sum over the workgroups' partials of entry e, in fp64 and a fixed order:
// slice s adds partials s, s + 32, ... ascending, the 32 slices are added ascending.
// A partial holds P = K*K + 2K entries (gram, rowsum, dist2) and with `tail` two more.
constexpr int kFinalEntries = 32, kFinalSlices = 32;
__global__ __launch_bounds__(kFinalEntries * kFinalSlices) void gram_final_kernel(
    const float* __restrict__ work, int64_t nparts, int K, double* __restrict__ gram, double* __restrict__ rowsum,
    double* __restrict__ dist2, double* __restrict__ tail) {
    __shared__ double red[kFinalSlices][kFinalEntries];
    const int P = K * K + 2 * K + (tail ? 2 : 0);
    const int ei = threadIdx.x % kFinalEntries, s = threadIdx.x / kFinalEntries;
    const int e = blockIdx.x * kFinalEntries + ei;
    double acc = 0.0;
    if (e < P) {
#pragma unroll 8
        for (int64_t w = s; w < nparts; w += kFinalSlices) acc += (double)work[w * P + e];
    }
    red[s][ei] = acc;
    __syncthreads();
    if (s == 0 && e < P) {
        double v = red[0][ei];
        for (int q = 1; q < kFinalSlices; ++q) v += red[q][ei];
        if (e < K * K) gram[e] = v;
        else if (e < K * K + K) rowsum[e - K * K] = v;
        else if (e >= K * K + 2 * K) tail[e - K * K - 2 * K] = v;
        else if (dist2) dist2[e - K * K - K] = v;
    }
}

static bool gram_aligned(const void* p, int bytes) { return ((uintptr_t)p % bytes) == 0; }

// CEN: gram = cgram, rowsum = dsum, dist2 = mdot, tail = mstat.
template <typename T, bool CEN>
static int launch_gram(const void* src, int64_t K, int64_t ld, int64_t n, double* gram, double* rowsum,
                       double* dist2, double* tail, void* work, hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = gram_aligned(src, vb) && (ld % 4 == 0 || K == 1);
    const int64_t grid = gram_grid(n);
    const int want = dist2 ? 1 : 0;
    const T* s = (const T*)src;
    float* w = (float*)work;
#define GA_GRAM_LAUNCH(KP, VEC)                                                                            \
    hipLaunchKernelGGL((gram_partial_kernel<T, KP, VEC, CEN>), dim3((unsigned)grid), dim3(kGramBlock), 0, \
                       stream, s, (int)K, ld, n, want, w)
    if (K > 16) {
        if (vec) GA_GRAM_LAUNCH(32, true);
        else GA_GRAM_LAUNCH(32, false);
    } else {
        if (vec) GA_GRAM_LAUNCH(16, true);
        else GA_GRAM_LAUNCH(16, false);
    }
#undef GA_GRAM_LAUNCH
    int rc = check_launch(CEN ? "ga_replica_gram_centered" : "ga_replica_gram");
    if (rc != GA_OK) return rc;
    const int P = (int)(CEN ? gram_centered_partial_len(K) : gram_partial_len(K));
    hipLaunchKernelGGL(gram_final_kernel, dim3((unsigned)ceil_div(P, kFinalEntries)),
                       dim3(kFinalEntries * kFinalSlices), 0, stream, (const float*)w, grid, (int)K, gram, rowsum,
                       dist2, tail);
    return check_launch(CEN ? "ga_replica_gram_centered (final sum)" : "ga_replica_gram (final sum)");
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int64_t ga_replica_gram_workspace_bytes(int64_t K, int64_t n) {
    if (K < 1 || K > kGramMaxK || n < 0) return -1;
    return gram_grid(n) * gram_partial_len(K) * (int64_t)sizeof(float);
}

extern "C" GA_API int ga_replica_gram_chain(void) { return kWaveCols; }

extern "C" GA_API int ga_replica_gram(int dtype, const void* src, int64_t K, int64_t ld, int64_t n, double* gram,
                                      double* rowsum, double* dist2, void* work, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_replica_gram: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    if (K > kGramMaxK) {
        set_error("ga_replica_gram: K=%lld replicas, at most %d are supported", (long long)K, kGramMaxK);
        return GA_EUNSUP;
    }
    GA_REQUIRE(dtype == GA_F32 || dtype == GA_BF16, "ga_replica_gram: unknown dtype %d", dtype);
    GA_REQUIRE(gram_aligned(gram, 8) && gram_aligned(rowsum, 8) && gram_aligned(dist2, 8) && gram_aligned(work, 4),
               "ga_replica_gram: outputs must be 8-byte aligned, the workspace 4-byte aligned");
    if (n == 0) {
        hipError_t e = hipSuccess;
        if (gram) e = hipMemsetAsync(gram, 0, (size_t)(K * K) * sizeof(double), stream);
        if (e == hipSuccess && rowsum) e = hipMemsetAsync(rowsum, 0, (size_t)K * sizeof(double), stream);
        if (e == hipSuccess && dist2) e = hipMemsetAsync(dist2, 0, (size_t)K * sizeof(double), stream);
        if (e != hipSuccess) {
            set_error("ga_replica_gram: hipMemsetAsync failed: %s", hipGetErrorString(e));
            return GA_EHIP;
        }
        return GA_OK;
    }
    GA_REQUIRE(src && gram && rowsum && work, "ga_replica_gram: null buffer");
    GA_REQUIRE(K == 1 || ld >= n, "ga_replica_gram: ld %lld < n %lld", (long long)ld, (long long)n);
    GA_REQUIRE(gram_aligned(src, dtype == GA_F32 ? 4 : 2), "ga_replica_gram: src is not element aligned");
    GA_REQUIRE(gram_grid(n) < (int64_t)INT32_MAX, "ga_replica_gram: n too large");
    if (dtype == GA_F32) return launch_gram<float, false>(src, K, ld, n, gram, rowsum, dist2, nullptr, work, stream);
    return launch_gram<__hip_bfloat16, false>(src, K, ld, n, gram, rowsum, dist2, nullptr, work, stream);
}

extern "C" GA_API int64_t ga_replica_gram_centered_workspace_bytes(int64_t K, int64_t n) {
    if (K < 1 || K > kGramMaxK || n < 0) return -1;
    return gram_grid(n) * gram_centered_partial_len(K) * (int64_t)sizeof(float);
}

extern "C" GA_API int ga_replica_gram_centered(int dtype, const void* src, int64_t K, int64_t ld, int64_t n,
                                               double* cgram, double* mdot, double* dsum, double* mstat,
                                               void* work, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_replica_gram_centered: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    if (K > kGramMaxK) {
        set_error("ga_replica_gram_centered: K=%lld replicas, at most %d are supported", (long long)K, kGramMaxK);
        return GA_EUNSUP;
    }
    GA_REQUIRE(dtype == GA_F32 || dtype == GA_BF16, "ga_replica_gram_centered: unknown dtype %d", dtype);
    GA_REQUIRE(gram_aligned(cgram, 8) && gram_aligned(mdot, 8) && gram_aligned(dsum, 8) && gram_aligned(mstat, 8) &&
                   gram_aligned(work, 4),
               "ga_replica_gram_centered: outputs must be 8-byte aligned, the workspace 4-byte aligned");
    if (n == 0) {
        hipError_t e = hipSuccess;
        if (cgram) e = hipMemsetAsync(cgram, 0, (size_t)(K * K) * sizeof(double), stream);
        if (e == hipSuccess && mdot) e = hipMemsetAsync(mdot, 0, (size_t)K * sizeof(double), stream);
        if (e == hipSuccess && dsum) e = hipMemsetAsync(dsum, 0, (size_t)K * sizeof(double), stream);
        if (e == hipSuccess && mstat) e = hipMemsetAsync(mstat, 0, 2 * sizeof(double), stream);
        if (e != hipSuccess) {
            set_error("ga_replica_gram_centered: hipMemsetAsync failed: %s", hipGetErrorString(e));
            return GA_EHIP;
        }
        return GA_OK;
    }
    GA_REQUIRE(src && cgram && mdot && dsum && mstat && work, "ga_replica_gram_centered: null buffer");
    GA_REQUIRE(K == 1 || ld >= n, "ga_replica_gram_centered: ld %lld < n %lld", (long long)ld, (long long)n);
    GA_REQUIRE(gram_aligned(src, dtype == GA_F32 ? 4 : 2), "ga_replica_gram_centered: src is not element aligned");
    GA_REQUIRE(gram_grid(n) < (int64_t)INT32_MAX, "ga_replica_gram_centered: n too large");
    if (dtype == GA_F32) return launch_gram<float, true>(src, K, ld, n, cgram, dsum, mdot, mstat, work, stream);
    return launch_gram<__hip_bfloat16, true>(src, K, ld, n, cgram, dsum, mdot, mstat, work, stream);
}
