// Top-k sparse DiLoCo pseudo-gradients: the k largest entries of every 4096-element
// chunk, with error feedback, as the wire (and memory) format of the outer step.
// Roofline: see DESIGN.md §3 "Sparse outer step" (the encode's search is VALU work).
//
// Format.  Chunks are 4096 consecutive elements of an arena row, nc = ceil(n / 4096),
// the last one may be short (length L < 4096); 1 <= k <= 256 entries per chunk.  One
// payload row per node, in bytes:
//   [ vals : nc * k x fp32 ][ idx : nc * k x uint16 ]      rounded up to 16 bytes
// Chunk c owns entries c*k .. c*k + k - 1 of both sections.  It emits min(k, L) real
// entries in ASCENDING INDEX ORDER (idx = offset inside the chunk, 0..4095); the
// remaining entries carry val = +0.0f, idx = 0xFFFF, which the decoder skips.  A chunk
// with fewer than k non-zeros still emits k entries (zeros are ordinary values).  The
// pad bytes behind the idx section are written as 0.
//
// Arithmetic.  Every line is one individually rounded fp32 operation (rn_add / rn_sub /
// rn_div below or an explicit fmaf, nothing contracted; tests/topk_checks.py does the
// same operations one at a time in numpy).
// Encode, row r, element i:
//   d   = master[i] - float(X[r, i])
//   d   = d + R[r, i]                              with a residual (error feedback)
//   key = bits(d) & 0x7fffffff                     (an integer: a total order, infinities
//                                                   and NaNs sort first, no special cases)
//   selected: the first min(k, L) elements of the chunk ordered by (key descending,
//   index ascending); ties at the k-th magnitude go to the lowest indices
//   payload value = d bit for bit;  R[r, i] = d - d where selected, d elsewhere
// Decode + outer step over S payload rows, per element:
//   acc = +0; for rows in ascending order that list the element: acc = acc + val
//   g = acc / divisor, then ga_diloco_outer's update of master / momentum on that g, the
//   new master written to K_out rows.  EVERY element is updated (momentum and weight
//   decay go on where acc = 0).
//
// topk_encode_kernel: one wavefront owns one chunk, a lane holds 64 keys in registers
// (register group j, element e: chunk offset 256 j + 4 lane + e, loaded as 16 vectors),
// the signs in 2 more.  The k-th key is found most significant bit first: a round counts
// key >= candidate with one ballot and scalar popcount per register (the count is
// wave-uniform as it forms: no cross-lane reduction), the search stops at the first
// candidate with exactly k keys at or above it.  Output ranks are lane prefixes
// of ballots (mbcnt) on a running wave-uniform base, entries are staged in LDS per wave
// and leave as coalesced stores; the residual is rewritten in the same pass.  The wave
// walks all K rows of its chunk with master kept in registers.  No atomics, no scratch.
// diloco_outer_sparse_kernel: one 256-thread workgroup owns one chunk: a 4096-float LDS
// accumulator takes the S rows' entries in ascending row order (indices are distinct
// within one row's chunk: plain read-modify-write, a barrier between rows, the loads of
// four rows in flight ahead of their barriers), then master / momentum stream through
// the update as in diloco_outer_dequant_kernel (sc1 stores).
#include "ga_common.h"

namespace ga {

constexpr int kTChunk = 4096;     // elements per chunk
constexpr int kTThreads = 256;    // 4 wavefronts
constexpr int kTWaves = kTThreads / 64;
constexpr int kTGroups = 16;      // register groups of a lane: 16 x 4 elements
constexpr int kTMaxK = 256;
constexpr uint32_t kTNoIdx = 0xFFFFu;

inline int64_t topk_chunks(int64_t n) { return ceil_div(n, kTChunk); }
inline int64_t topk_row_bytes(int64_t n, int k) { return (topk_chunks(n) * k * 6 + 15) / 16 * 16; }

// One correctly rounded fp32 operation that no neighbour can be fused into (quant.hip's
// pattern: hipcc contracts a * b + c across statements by default).
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

// Set bits of m below this lane.
__device__ __forceinline__ int lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// LDS written by some lanes of a wave and read by others of the same wave.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// X: [K, ld_x] rows of T, master: [n] fp32, R: [K, ld_r] fp32 or null, payload: [K, ld_q] bytes.
// VEC: 16-byte (bf16: 8-byte) loads and stores on whole chunks; the short last chunk, and
// every chunk when VEC is false, goes element by element with the same arithmetic.
template <typename T, bool VEC>
__global__ __launch_bounds__(kTThreads) void topk_encode_kernel(
    const T* __restrict__ X, int64_t K, int64_t ld_x, const float* __restrict__ master, float* __restrict__ R,
    int64_t ld_r, int64_t n, int k, uint8_t* __restrict__ payload, int64_t ld_q) {
    using V = typename Vec4<T>::type;
    __shared__ float s_val[kTWaves][kTMaxK];
    __shared__ uint16_t s_idx[kTWaves][kTMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nc = (n + kTChunk - 1) / kTChunk;
    const int64_t c = (int64_t)blockIdx.x * kTWaves + wave;  // wave-uniform
    if (c >= nc) return;                                     // no workgroup barrier below
    const int64_t base = c * kTChunk;
    const int L = n - base < kTChunk ? (int)(n - base) : kTChunk;
    const bool whole = VEC && L == kTChunk;
    const int64_t entries = nc * k;                          // per section
    const int64_t row_bytes = (entries * 6 + 15) / 16 * 16;

    float m[4 * kTGroups];
#pragma unroll
    for (int j = 0; j < kTGroups; ++j) {
        const int o = 256 * j + 4 * lane;
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        if (whole) {
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(master + base + o)), f);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (o + e < L) f[e] = master[base + o + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) m[4 * j + e] = f[e];
    }

    for (int64_t r = 0; r < K; ++r) {
        const T* x = X + r * ld_x + base;
        float* res = R ? R + r * ld_r + base : nullptr;
        // keys >= 0 of the elements inside the chunk, -1 past its end; the signs apart
        int key[4 * kTGroups];
        uint32_t sign[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < kTGroups; ++j) {
            const int o = 256 * j + 4 * lane;
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (whole) {
                float f[4];
                Vec4<T>::unpack(stream_load(reinterpret_cast<const V*>(x + o)), f);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = rn_sub(m[4 * j + e], f[e]);
                if (res) {
                    Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(res + o)), f);
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = rn_add(d[e], f[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (o + e < L) {
                        d[e] = rn_sub(m[4 * j + e], Elem<T>::load(x + o + e));
                        if (res) d[e] = rn_add(d[e], res[o + e]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 4 * j + e;
                const uint32_t u = __float_as_uint(d[e]);
                key[p] = (whole || o + e < L) ? (int)(u & 0x7fffffffu) : -1;
                sign[p >> 5] |= (u >> 31) << (p & 31);
            }
        }

        // the k-th largest key, most significant bit first; thr stays 0 when L < k
        int thr = 0;
        for (int b = 30; b >= 0; --b) {
            const int cand = thr | (1 << b);
            int tot = 0;  // counted on the scalar unit: a ballot and its popcount per register
#pragma unroll
            for (int p = 0; p < 4 * kTGroups; ++p) tot += __popcll(__ballot(key[p] >= cand));
            if (tot >= k) {
                thr = cand;
                if (tot == k) break;  // exactly the k keys at or above cand: nothing left to resolve
            }
        }
        int gt = 0;
#pragma unroll
        for (int p = 0; p < 4 * kTGroups; ++p) gt += __popcll(__ballot(key[p] > thr));
        const int need = k - gt;  // how many keys equal to thr are admitted, lowest indices first

        wave_lds_sync();  // the previous row's staged entries have been read
        int out_base = 0, eq_base = 0;  // wave-uniform: entries / equal keys in the groups before j
#pragma unroll
        for (int j = 0; j < kTGroups; ++j) {
            const int o = 256 * j + 4 * lane;
            uint64_t bq[4];
            int eq_rank = eq_base;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bq[e] = __ballot(key[4 * j + e] == thr);
                eq_rank += lanes_below(bq[e]);
            }
            bool sel[4];
            uint64_t bs[4];
            int pos = out_base;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool eq = key[4 * j + e] == thr;
                sel[e] = key[4 * j + e] > thr || (eq && eq_rank < need);
                eq_rank += eq ? 1 : 0;
                bs[e] = __ballot(sel[e]);
                pos += lanes_below(bs[e]);
            }
            float d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 4 * j + e;
                d[e] = __uint_as_float((uint32_t)key[p] | (((sign[p >> 5] >> (p & 31)) & 1u) << 31));
                if (sel[e]) {  // pos < k: at most k elements are selected
                    s_val[wave][pos] = d[e];
                    s_idx[wave][pos] = (uint16_t)(o + e);
                    ++pos;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                eq_base += __popcll(bq[e]);
                out_base += __popcll(bs[e]);
            }
            if (res) {
                float w[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = sel[e] ? rn_sub(d[e], d[e]) : d[e];
                if (whole) {
                    stream_store(reinterpret_cast<float4*>(res + o), Vec4<float>::pack(w));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (o + e < L) res[o + e] = w[e];
                }
            }
        }
        // a chunk shorter than k: the entries that stay empty
        for (int t = out_base + lane; t < k; t += 64) {
            s_val[wave][t] = 0.f;
            s_idx[wave][t] = (uint16_t)kTNoIdx;
        }
        wave_lds_sync();
        uint8_t* row = payload + r * ld_q;
        float* pv = reinterpret_cast<float*>(row) + c * k;
        uint16_t* pi = reinterpret_cast<uint16_t*>(row + entries * 4) + c * k;
        for (int t = lane; t < k; t += 64) {
            pv[t] = s_val[wave][t];
            pi[t] = s_idx[wave][t];
        }
        // the pad behind the idx section (0 .. 14 bytes), by the wave of the last chunk
        if (c == nc - 1) {
            const int pad = (int)(row_bytes - entries * 6) >> 1;
            if (lane < pad) reinterpret_cast<uint16_t*>(row + entries * 6)[lane] = 0;
        }
    }
}

// ga_diloco_outer's element update from the pseudo-gradient on, the sequence of
// quant.hip's quant_outer_update.
struct SparseOuterParams {
    float divisor, lr, momentum, dampening, weight_decay;
    int first_step, nesterov;
};

__device__ __forceinline__ float sparse_outer_update(float acc, float& master, float& buf,
                                                     const SparseOuterParams& op) {
    float g = rn_div(acc, op.divisor);
    if (op.weight_decay != 0.f) g = fmaf(op.weight_decay, master, g);
    if (op.momentum != 0.f) {
        if (op.first_step) buf = g;
        else buf = fmaf(rn_sub(1.f, op.dampening), g, rn_mul(buf, op.momentum));
        g = op.nesterov ? fmaf(op.momentum, buf, g) : buf;
    }
    master = fmaf(-op.lr, g, master);
    return master;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kTThreads) void diloco_outer_sparse_kernel(
    const uint8_t* __restrict__ payload, int64_t S, int64_t ld_q, int k, int64_t n, float* master, float* mom,
    SparseOuterParams op, T* dst, int64_t K_out, int64_t ld_dst) {
    __shared__ __attribute__((aligned(16))) float acc[kTChunk];
    const int tid = threadIdx.x;
    const bool has_mom = op.momentum != 0.f;
    const int64_t nc = (n + kTChunk - 1) / kTChunk;
    const int64_t c = blockIdx.x;
    const int64_t base = c * kTChunk;
    const int L = n - base < kTChunk ? (int)(n - base) : kTChunk;
#pragma unroll
    for (int i = 0; i < kTChunk / 4 / kTThreads; ++i)
        reinterpret_cast<float4*>(acc)[tid + kTThreads * i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    // thread t owns entry t of the chunk in every row; rows in ascending order, a barrier
    // after each, the loads of four rows issued ahead of their barriers
    const int64_t ent = c * k + tid;
    const int64_t idx_off = nc * k * 4;
    const bool act = tid < k;
    for (int64_t r = 0; r < S; r += 4) {
        float v[4];
        uint32_t ix[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = 0.f;
            ix[u] = kTNoIdx;
            if (act && r + u < S) {
                const uint8_t* row = payload + (r + u) * ld_q;
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const float*>(row) + ent);
                ix[u] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(row + idx_off) + ent);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r + u < S) {  // uniform
                if (ix[u] < (uint32_t)kTChunk) acc[ix[u]] = rn_add(acc[ix[u]], v[u]);  // 0xFFFF: an empty entry
                __syncthreads();
            }
        }
    }

    if (VEC && L == kTChunk) {
        using V = typename Vec4<T>::type;
        float4* m4 = reinterpret_cast<float4*>(master + base);
        float4* b4 = has_mom ? reinterpret_cast<float4*>(mom + base) : nullptr;
#pragma unroll
        for (int i = 0; i < kTChunk / 4 / kTThreads; ++i) {
            const uint32_t vi = (uint32_t)(tid + kTThreads * i);
            float a[4], m[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            Vec4<float>::unpack(reinterpret_cast<const float4*>(acc)[vi], a);
            Vec4<float>::unpack(stream_load(m4 + vi), m);
            if (has_mom && !op.first_step) Vec4<float>::unpack(stream_load(b4 + vi), b);
            float out[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = sparse_outer_update(a[e], m[e], b[e], op);
            const V o = Vec4<T>::pack(out);
            // device-scope (sc1) stores based at the workgroup's chunk of each stream
            store_sc1(m4, vi, Vec4<float>::pack(m));
            if (has_mom) store_sc1(b4, vi, Vec4<float>::pack(b));
            for (int64_t j = 0; j < K_out; ++j) store_sc1(reinterpret_cast<V*>(dst + j * ld_dst + base), vi, o);
        }
    } else {
        for (int i = tid; i < L; i += kTThreads) {
            float m = master[base + i];
            float b = (has_mom && !op.first_step) ? mom[base + i] : 0.f;
            const float out = sparse_outer_update(acc[i], m, b, op);
            master[base + i] = m;
            if (has_mom) mom[base + i] = b;
            for (int64_t j = 0; j < K_out; ++j) Elem<T>::store(dst + j * ld_dst + base + i, out);
        }
    }
}

static bool t_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

template <typename T>
static int launch_topk_encode(const void* x, int64_t K, int64_t ld_x, const float* master, float* residual,
                              int64_t ld_r, int64_t n, int k, uint8_t* payload, int64_t ld_q, hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = t_aligned(x, vb) && (K == 1 || ld_x % 4 == 0) && t_aligned(master, 16) &&
                     t_aligned(residual, 16) && (K == 1 || residual == nullptr || ld_r % 4 == 0);
    const dim3 grid((unsigned)ceil_div(topk_chunks(n), kTWaves));
    if (vec)
        hipLaunchKernelGGL((topk_encode_kernel<T, true>), grid, dim3(kTThreads), 0, stream, (const T*)x, K, ld_x,
                           master, residual, ld_r, n, k, payload, ld_q);
    else
        hipLaunchKernelGGL((topk_encode_kernel<T, false>), grid, dim3(kTThreads), 0, stream, (const T*)x, K, ld_x,
                           master, residual, ld_r, n, k, payload, ld_q);
    return check_launch("ga_topk_encode");
}

template <typename T>
static int launch_outer_sparse(const uint8_t* payload, int64_t S, int64_t ld_q, int k, int64_t n, float* master,
                               float* mom, const SparseOuterParams& op, void* dst, int64_t K_out, int64_t ld_dst,
                               hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = (K_out <= 1 || ld_dst % 4 == 0) && t_aligned(dst, vb) && t_aligned(master, 16) &&
                     t_aligned(mom, 16);
    const dim3 grid((unsigned)topk_chunks(n));
    if (vec)
        hipLaunchKernelGGL((diloco_outer_sparse_kernel<T, true>), grid, dim3(kTThreads), 0, stream, payload, S, ld_q,
                           k, n, master, mom, op, (T*)dst, K_out, ld_dst);
    else
        hipLaunchKernelGGL((diloco_outer_sparse_kernel<T, false>), grid, dim3(kTThreads), 0, stream, payload, S, ld_q,
                           k, n, master, mom, op, (T*)dst, K_out, ld_dst);
    return check_launch("ga_diloco_outer_sparse");
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int64_t ga_topk_row_bytes(int64_t n, int k) {
    if (n < 0 || k < 1 || k > kTMaxK) return -1;
    return topk_row_bytes(n, k);
}

extern "C" GA_API int ga_topk_encode(int dtype, const void* x, int64_t K, int64_t ld_x, const float* master,
                                     float* residual, int64_t ld_r, int64_t n, int k, void* payload,
                                     int64_t ld_q_bytes, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_topk_encode: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    GA_REQUIRE(k >= 1 && k <= kTMaxK, "ga_topk_encode: k %d is not in 1..%d", k, kTMaxK);
    if (n == 0) return GA_OK;
    GA_REQUIRE(x && master && payload, "ga_topk_encode: null x/master/payload");
    GA_REQUIRE(K == 1 || ld_x >= n, "ga_topk_encode: ld_x < n");
    GA_REQUIRE(K == 1 || residual == nullptr || ld_r >= n, "ga_topk_encode: ld_r < n");
    GA_REQUIRE(ld_q_bytes >= topk_row_bytes(n, k) && ld_q_bytes % 16 == 0,
               "ga_topk_encode: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)topk_row_bytes(n, k));
    GA_REQUIRE(t_aligned(payload, 16), "ga_topk_encode: the payload is not 16-byte aligned");
    GA_REQUIRE(t_aligned(master, 4) && t_aligned(residual, 4), "ga_topk_encode: master/residual not 4-byte aligned");
    uint8_t* pl = (uint8_t*)payload;
    switch (dtype) {
        case GA_F32:
            return launch_topk_encode<float>(x, K, ld_x, master, residual, ld_r, n, k, pl, ld_q_bytes, stream);
        case GA_BF16:
            GA_REQUIRE(t_aligned(x, 2), "ga_topk_encode: x is not 2-byte aligned");
            return launch_topk_encode<__hip_bfloat16>(x, K, ld_x, master, residual, ld_r, n, k, pl, ld_q_bytes, stream);
        default:
            set_error("ga_topk_encode: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_sparse(const void* payload, int64_t S, int64_t ld_q_bytes, int k, int64_t n,
                                             float divisor, float* master, float* mom, int first_step, float lr,
                                             float momentum, float dampening, float weight_decay, int nesterov,
                                             int dtype, void* dst, int64_t K_out, int64_t ld_dst,
                                             hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && S >= 1 && K_out >= 0, "ga_diloco_outer_sparse: bad sizes n=%lld S=%lld K_out=%lld",
               (long long)n, (long long)S, (long long)K_out);
    GA_REQUIRE(k >= 1 && k <= kTMaxK, "ga_diloco_outer_sparse: k %d is not in 1..%d", k, kTMaxK);
    if (n == 0) return GA_OK;
    GA_REQUIRE(payload && master, "ga_diloco_outer_sparse: null payload/master");
    GA_REQUIRE(K_out == 0 || dst, "ga_diloco_outer_sparse: null dst");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_sparse: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(K_out <= 1 || ld_dst >= n, "ga_diloco_outer_sparse: ld_dst < n");
    GA_REQUIRE(ld_q_bytes >= topk_row_bytes(n, k) && ld_q_bytes % 16 == 0,
               "ga_diloco_outer_sparse: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)topk_row_bytes(n, k));
    GA_REQUIRE(t_aligned(payload, 16), "ga_diloco_outer_sparse: the payload is not 16-byte aligned");
    GA_REQUIRE(t_aligned(master, 4) && t_aligned(mom, 4), "ga_diloco_outer_sparse: master/mom not 4-byte aligned");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_sparse: divisor is 0");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_sparse: Nesterov momentum requires a momentum and zero dampening");
    SparseOuterParams op{divisor, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    const uint8_t* pl = (const uint8_t*)payload;
    switch (dtype) {
        case GA_F32:
            return launch_outer_sparse<float>(pl, S, ld_q_bytes, k, n, master, mom, op, dst, K_out, ld_dst, stream);
        case GA_BF16:
            return launch_outer_sparse<__hip_bfloat16>(pl, S, ld_q_bytes, k, n, master, mom, op, dst, K_out, ld_dst,
                                                       stream);
        default:
            set_error("ga_diloco_outer_sparse: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}
