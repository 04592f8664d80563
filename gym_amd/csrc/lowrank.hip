// Low-rank (PowerSGD) DiLoCo pseudo-gradients: the outer step whose exchange is two
// all-reduces of rank-r factors, flat in the world size.  Roofline: HBM (DESIGN.md §3
// "Low-rank outer step"); the two tall-skinny products run on the f32 MFMA.
//
// Plan (built once on the host, gym_amd/lowrank.py).  tensors: int64 rows
//   {off, m, n, kind, poff, qoff}: the tensor at arena offset `off` viewed as the row-major
//   m x n matrix, kind 1 = compressed (P_t = A[poff .. poff + m r), Q_t = Q[qoff .. qoff + n r),
//   both row-major with r columns), kind 0 = dense.  segments: int64 rows {off, len, aoff}: a
//   run of dense elements (dense tensors and padding) whose sums live at A[aoff .. aoff + len);
//   off and aoff are multiples of 4.  jobs: int32 rows {id, band, tile, 0}, one workgroup each:
//   id >= 0 a compressed tensor, id < 0 segment -1 - id with band = its 4096-element chunk.
//
// project      job = (tensor, 32 rows): the four waves take the band's 64-column tiles in turn
//              (wave w tiles w, w + 4, ..).  A tile of the summed delta sum_k (master - x_k) + e_k
//              is formed in registers from coalesced loads (16 lanes x float4 = 64 columns of a
//              row, 4 rows per instruction), stored to the wave's LDS image [row][column] and
//              read back with the row on the lane -- the A operand of v_mfma_f32_32x32x2_f32;
//              Q's 64 x r slab is staged transposed [c][j] (rows c >= r zero) and read the same
//              way as the B operand.  The waves' 32 x 32 results are added in wave order.
// backproject  job = (tensor, 32 columns): lanes lie along the columns, so the coalesced load of
//              a row's 32 columns IS the A operand of M^T; P-hat's row is the B operand.  A wave
//              takes 16 rows (8 MFMAs) per step, the waves take the steps in turn.
// orthonormalize  one workgroup of 1024 threads per compressed tensor, thread i owns rows
//              i, i + 1024, .. through every sweep (so only the reductions synchronise); columns
//              stay in global memory / L2.
// outer        job = (tensor, 32 rows, 128 columns) or a dense chunk: P-hat's 32 rows and Q's
//              128 rows go to LDS once, a thread forms g for 4 rows x 4 columns.
//
// Determinism: no atomics, every output element has one owner, every reduction a fixed order.
// Chain bound (ga_lowrank_chain): an MFMA accumulator of the project takes 64 multiply-adds
// per tile and ceil(tiles / 4) tiles, of the back-projection 16 per step and ceil(steps / 4).
#include "ga_common.h"
#include "quant_math.h"  // rn_*, QuantOuterParams, outer_update_from_g

namespace ga {

constexpr int kLrThreads = 256;
constexpr int kLrWaves = kLrThreads / 64;
constexpr int kLrBand = 32;                  // rows (project, outer) or columns (back-project) of a job
constexpr int kLrTile = 64;                  // columns of a project tile
constexpr int kLrStride = kLrTile + 4;       // LDS row stride of the project images, 16-B aligned rows
constexpr int kLrStep = 16;                  // rows of a back-project step
constexpr int kLrMaxRank = 32;
constexpr int64_t kLrChunk = 4096;           // elements of a dense job
constexpr int kLrOutCols = 128;              // columns of an outer job
constexpr int kLrOutStride = kLrOutCols + 4;
constexpr int kLrOrthThreads = 1024;
constexpr int kLrOrthWaves = kLrOrthThreads / 64;
constexpr int kLrFields = 6;

typedef float lr_f16v __attribute__((ext_vector_type(16)));

// The K local rows with the master and the residual: what a delta is formed from.
struct LrRows {
    const float* x;
    int64_t K, ld_x;
    const float* master;
    const float* resid;  // null: no error feedback
    int64_t ld_r;
};

struct LrTensor {
    int64_t off, m, n, kind, poff, qoff;
};
__device__ __forceinline__ LrTensor lr_tensor(const int64_t* tens, int t) {
    const int64_t* p = tens + (int64_t)t * kLrFields;
    return LrTensor{p[0], p[1], p[2], p[3], p[4], p[5]};
}

// Elements [0, valid) of the four at p; vec: p is 16-byte aligned.
__device__ __forceinline__ float4 lr_load4(const float* p, bool vec, int valid) {
    if (vec && valid >= 4) return stream_load(reinterpret_cast<const float4*>(p));
    float f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < valid) f[e] = __builtin_nontemporal_load(p + e);
    return make_float4(f[0], f[1], f[2], f[3]);
}
__device__ __forceinline__ void lr_store4(float* p, bool vec, int valid, const float4& v) {
    if (vec && valid >= 4) {
        stream_store(reinterpret_cast<float4*>(p), v);
        return;
    }
    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < valid) __builtin_nontemporal_store(f[e], p + e);
}

// M_k = (master - x_k) + e_k, one rounded operation each.
__device__ __forceinline__ float lr_delta(float m, float x, float e) { return rn_add(rn_sub(m, x), e); }

// sum over the local rows, ascending k from 0, of M_k at elements idx .. idx + 3
__device__ __forceinline__ float4 lr_delta_sum4(const LrRows& R, int64_t idx, bool vec, int valid) {
    const float4 m = lr_load4(R.master + idx, vec, valid);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
    for (int64_t k = 0; k < R.K; ++k) {
        const float4 x = lr_load4(R.x + k * R.ld_x + idx, vec, valid);
        float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
        if (R.resid) e = lr_load4(R.resid + k * R.ld_r + idx, vec, valid);
        acc.x = rn_add(acc.x, lr_delta(m.x, x.x, e.x));
        acc.y = rn_add(acc.y, lr_delta(m.y, x.y, e.y));
        acc.z = rn_add(acc.z, lr_delta(m.z, x.z, e.z));
        acc.w = rn_add(acc.w, lr_delta(m.w, x.w, e.w));
    }
    return acc;
}
__device__ __forceinline__ float lr_delta_sum1(const LrRows& R, int64_t idx) {
    const float m = __builtin_nontemporal_load(R.master + idx);
    float acc = 0.f;
#pragma unroll 2
    for (int64_t k = 0; k < R.K; ++k) {
        const float x = __builtin_nontemporal_load(R.x + k * R.ld_x + idx);
        const float e = R.resid ? __builtin_nontemporal_load(R.resid + k * R.ld_r + idx) : 0.f;
        acc = rn_add(acc, lr_delta(m, x, e));
    }
    return acc;
}

__device__ __forceinline__ void lr_wave_lds_sync() {
    // the image is private to the wave: its LDS operations complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The four waves' 32 x 32 MFMA results (register e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5),
// column l & 31) through LDS, added in wave order; rows < nrows, columns < r go to out[row * r + c].
// img: the waves' images, `stride` floats apart, at least 32 x 32 each.
__device__ __forceinline__ void lr_reduce_store(float* img, int stride, const lr_f16v& acc, int r, int64_t nrows,
                                                float* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        img[wave * stride + row * 32 + (lane & 31)] = acc[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kLrBand * r; i += kLrThreads) {
        const int row = i / r, c = i - row * r;
        float v = img[row * 32 + c];
#pragma unroll
        for (int w = 1; w < kLrWaves; ++w) v = rn_add(v, img[w * stride + row * 32 + c]);
        if (row < nrows) out[(int64_t)row * r + c] = v;
    }
}

// Dense chunk of the project: A[aoff + i] = the ascending fp32 sum of the local x_k[off + i].
__device__ __forceinline__ void lr_dense_sum(const int64_t* seg, int chunk, const LrRows& R, bool vec, float* A) {
    const int64_t off = seg[0], len = seg[1], aoff = seg[2];
    const int64_t lo = (int64_t)chunk * kLrChunk, hi = lo + kLrChunk < len ? lo + kLrChunk : len;
    for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * kLrThreads) {
        const int valid = hi - i < 4 ? (int)(hi - i) : 4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int64_t k = 0; k < R.K; ++k) {
            const float4 x = lr_load4(R.x + k * R.ld_x + off + i, vec, valid);
            acc.x = rn_add(acc.x, x.x);
            acc.y = rn_add(acc.y, x.y);
            acc.z = rn_add(acc.z, x.z);
            acc.w = rn_add(acc.w, x.w);
        }
        lr_store4(A + aoff + i, vec, valid, acc);
    }
}

__global__ __launch_bounds__(kLrThreads) void lowrank_project_kernel(
    const int4* __restrict__ jobs, const int64_t* __restrict__ tens, const int64_t* __restrict__ segs, LrRows R,
    const float* __restrict__ Q, float q_div, int r, int aligned, float* __restrict__ A) {
    __shared__ __attribute__((aligned(16))) float img[kLrWaves][kLrBand * kLrStride];
    __shared__ __attribute__((aligned(16))) float qim[kLrWaves][kLrBand * kLrStride];
    const int4 job = jobs[blockIdx.x];
    if (job.x < 0) {
        lr_dense_sum(segs + (int64_t)(-1 - job.x) * 3, job.y, R, aligned != 0, A);
        return;
    }
    const LrTensor T = lr_tensor(tens, job.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)job.y * kLrBand;
    const bool vec = aligned && (T.n & 3) == 0;  // off is a multiple of 4: every row then starts 16-byte aligned
    float* my = img[wave];
    float* myq = qim[wave];
    for (int c = r; c < kLrBand; ++c) myq[c * kLrStride + lane] = 0.f;  // columns >= r of Q
    lr_f16v acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int64_t ntiles = (T.n + kLrTile - 1) / kLrTile;
    for (int64_t tile = wave; tile < ntiles; tile += kLrWaves) {  // wave-uniform
        const int64_t j0 = tile * kLrTile;
        const int64_t col = j0 + 4 * (lane & 15);
        const int valid = T.n - col < 4 ? (int)(T.n - col) : 4;
#pragma unroll
        for (int p = 0; p < kLrBand / 4; ++p) {
            const int rl = 4 * p + (lane >> 4);
            const int64_t row = row0 + rl;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < T.m && valid > 0) d = lr_delta_sum4(R, T.off + row * T.n + col, vec, valid);
            *reinterpret_cast<float4*>(my + rl * kLrStride + 4 * (lane & 15)) = d;
        }
        // Q's rows j0 .. j0 + 63 (contiguous, r values each) transposed to [c][j]; rows past n are 0
        const int64_t left = T.n - j0 < kLrTile ? T.n - j0 : kLrTile;
        const int have = (int)left * r;
        const float* qs = Q + T.qoff + j0 * r;
        for (int s = 0; s < r; ++s) {
            const int i = lane + 64 * s;
            const int j = i / r, c = i - j * r;
            myq[c * kLrStride + j] = i < have ? rn_div(qs[i], q_div) : 0.f;
        }
        lr_wave_lds_sync();
        // lane (i = l & 31, h = l >> 5): columns 8q + 4h + e; MFMA e of step q sums columns 8q + e and 8q + 4 + e
        const float* ra = my + (lane & 31) * kLrStride + 4 * (lane >> 5);
        const float* rb = myq + (lane & 31) * kLrStride + 4 * (lane >> 5);
#pragma unroll 4
        for (int q = 0; q < kLrTile / 8; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(ra + 8 * q);
            const float4 b = *reinterpret_cast<const float4*>(rb + 8 * q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        lr_wave_lds_sync();
    }
    lr_reduce_store(&img[0][0], kLrBand * kLrStride, acc, r, T.m - row0, A + T.poff + row0 * r);
}

__global__ __launch_bounds__(kLrThreads) void lowrank_backproject_kernel(
    const int4* __restrict__ jobs, const int64_t* __restrict__ tens, LrRows R, const float* __restrict__ A, int r,
    float* __restrict__ B) {
    __shared__ float img[kLrWaves][kLrBand * kLrBand];  // the final wave-order sum only
    const int4 job = jobs[blockIdx.x];
    const LrTensor T = lr_tensor(tens, job.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j0 = (int64_t)job.y * kLrBand;
    const int64_t j = j0 + (lane & 31);
    const int c = lane & 31, h = lane >> 5;
    const float* P = A + T.poff;
    lr_f16v acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int64_t nsteps = (T.m + kLrStep - 1) / kLrStep;
    for (int64_t s = wave; s < nsteps; s += kLrWaves) {  // wave-uniform
        float a[kLrStep / 2], b[kLrStep / 2];
#pragma unroll
        for (int u = 0; u < kLrStep / 2; ++u) {
            const int64_t row = s * kLrStep + 2 * u + h;
            a[u] = (row < T.m && j < T.n) ? lr_delta_sum1(R, T.off + row * T.n + j) : 0.f;
            b[u] = (row < T.m && c < r) ? P[row * r + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kLrStep / 2; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
    }
    lr_reduce_store(&img[0][0], kLrBand * kLrBand, acc, r, T.n - j0, B + T.qoff + j0 * r);
}

// Fixed-order sum over the workgroup: xor butterfly inside a wave (every lane ends with the
// same value), then the waves' values ascending.  red: [kLrOrthWaves] floats of this value.
__device__ __forceinline__ float lr_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = rn_add(v, __shfl_xor(v, o, 64));
    return v;
}

// dot[b], b < cnt, and extra: every thread returns with the workgroup's sums.
__device__ __forceinline__ void lr_block_sums(float (&dot)[kLrMaxRank], int cnt, float& extra,
                                              float (*red)[kLrOrthWaves]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int b = 0; b < kLrMaxRank; ++b) {
        if (b < cnt) {
            const float v = lr_wave_sum(dot[b]);
            if (lane == 0) red[b][wave] = v;
        }
    }
    const float x = lr_wave_sum(extra);
    if (lane == 0) red[kLrMaxRank][wave] = x;
    __syncthreads();
#pragma unroll
    for (int b = 0; b < kLrMaxRank; ++b) {
        if (b < cnt) {
            float v = red[b][0];
            for (int w = 1; w < kLrOrthWaves; ++w) v = rn_add(v, red[b][w]);
            dot[b] = v;
        }
    }
    float v = red[kLrMaxRank][0];
    for (int w = 1; w < kLrOrthWaves; ++w) v = rn_add(v, red[kLrMaxRank][w]);
    extra = v;
    __syncthreads();
}

// Classical Gram-Schmidt with a second projection (CGS2), column by column, in place.
__global__ __launch_bounds__(kLrOrthThreads) void lowrank_orth_kernel(const int64_t* __restrict__ tens, int r,
                                                                      float* A) {
    __shared__ float red[kLrMaxRank + 1][kLrOrthWaves];
    const LrTensor T = lr_tensor(tens, blockIdx.x);
    if (T.kind == 0) return;  // uniform over the workgroup
    float* P = A + T.poff;
    const int64_t m = T.m;
    for (int c = 0; c < r; ++c) {
        float dot[kLrMaxRank];
#pragma unroll
        for (int b = 0; b < kLrMaxRank; ++b) dot[b] = 0.f;
        // sweep 1: the column's squared norm and its products with the earlier columns
        float n0 = 0.f;
        for (int64_t i = threadIdx.x; i < m; i += kLrOrthThreads) {
            const float* row = P + i * r;
            const float v = row[c];
            n0 = fmaf(v, v, n0);
#pragma unroll
            for (int b = 0; b < kLrMaxRank; ++b)
                if (b < c) dot[b] = fmaf(v, row[b], dot[b]);
        }
        lr_block_sums(dot, c, n0, red);
        // sweeps 2 and 3: take the products off (ascending b), sweep 2 also forms the products of
        // what is left with the earlier columns, sweep 3 its squared norm
        float n2 = 0.f;
        for (int pass = 0; pass < 2; ++pass) {
            float next[kLrMaxRank];
#pragma unroll
            for (int b = 0; b < kLrMaxRank; ++b) next[b] = 0.f;
            n2 = 0.f;
            for (int64_t i = threadIdx.x; i < m; i += kLrOrthThreads) {
                float* row = P + i * r;
                float v = row[c];
#pragma unroll
                for (int b = 0; b < kLrMaxRank; ++b)
                    if (b < c) v = fmaf(-dot[b], row[b], v);
                row[c] = v;
                n2 = fmaf(v, v, n2);
                if (pass == 0) {
#pragma unroll
                    for (int b = 0; b < kLrMaxRank; ++b)
                        if (b < c) next[b] = fmaf(v, row[b], next[b]);
                }
            }
            lr_block_sums(next, pass == 0 ? c : 0, n2, red);
#pragma unroll
            for (int b = 0; b < kLrMaxRank; ++b) dot[b] = next[b];
        }
        // sweep 4: normalise, or drop a column that is zero or noise of the earlier ones
        const bool dead = !(n2 > 0.f) || n2 <= rn_mul(0x1p-40f, n0);
        const float len = sqrtf(n2);
        for (int64_t i = threadIdx.x; i < m; i += kLrOrthThreads) {
            float* row = P + i * r;
            row[c] = dead ? 0.f : rn_div(row[c], len);
        }
    }
}

__global__ __launch_bounds__(kLrThreads) void diloco_outer_lowrank_kernel(
    const int4* __restrict__ jobs, const int64_t* __restrict__ tens, const int64_t* __restrict__ segs,
    const float* __restrict__ A, const float* __restrict__ Q, float q_div, int r, float* x, int64_t K, int64_t ld_x,
    float* resid, int64_t ld_r, float* master, float* mom, QuantOuterParams op, float ktotal, int aligned) {
    __shared__ float ps[kLrBand * kLrMaxRank];
    __shared__ __attribute__((aligned(16))) float qs[kLrMaxRank * kLrOutStride];
    const bool has_mom = op.momentum != 0.f;
    const bool load_mom = has_mom && !op.first_step;
    const int4 job = jobs[blockIdx.x];
    if (job.x < 0) {
        // dense: g = master - S / K_total, ga_diloco_outer's arithmetic
        const int64_t* seg = segs + (int64_t)(-1 - job.x) * 3;
        const int64_t off = seg[0], len = seg[1], aoff = seg[2];
        const int64_t lo = (int64_t)job.y * kLrChunk, hi = lo + kLrChunk < len ? lo + kLrChunk : len;
        const bool vec = aligned != 0;
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * kLrThreads) {
            const int valid = hi - i < 4 ? (int)(hi - i) : 4;
            float s[4], m[4], b[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
            Vec4<float>::unpack(lr_load4(A + aoff + i, vec, valid), s);
            Vec4<float>::unpack(lr_load4(master + off + i, vec, valid), m);
            if (load_mom) Vec4<float>::unpack(lr_load4(mom + off + i, vec, valid), b);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                out[e] = outer_update_from_g(rn_sub(m[e], rn_div(s[e], ktotal)), m[e], b[e], op);
            lr_store4(master + off + i, vec, valid, Vec4<float>::pack(m));
            if (has_mom) lr_store4(mom + off + i, vec, valid, Vec4<float>::pack(b));
            const float4 o = Vec4<float>::pack(out);
            for (int64_t k = 0; k < K; ++k) lr_store4(x + k * ld_x + off + i, vec, valid, o);
        }
        return;
    }
    const LrTensor T = lr_tensor(tens, job.x);
    const int64_t row0 = (int64_t)job.y * kLrBand, c0 = (int64_t)job.z * kLrOutCols;
    const bool vec = aligned && (T.n & 3) == 0;
    {
        const int64_t rows = T.m - row0 < kLrBand ? T.m - row0 : kLrBand;
        const float* src = A + T.poff + row0 * r;
        for (int i = threadIdx.x; i < kLrBand * r; i += kLrThreads) {
            const int row = i / r, c = i - row * r;
            ps[row * kLrMaxRank + c] = row < rows ? src[i] : 0.f;
        }
        const int64_t cols = T.n - c0 < kLrOutCols ? T.n - c0 : kLrOutCols;
        const float* qsrc = Q + T.qoff + c0 * r;
        for (int i = threadIdx.x; i < kLrOutCols * r; i += kLrThreads) {
            const int j = i / r, c = i - j * r;
            qs[c * kLrOutStride + j] = j < cols ? rn_div(qsrc[i], q_div) : 0.f;
        }
    }
    __syncthreads();
    const int cl = 4 * (threadIdx.x & 31), rsub = threadIdx.x >> 5;
    const int64_t col = c0 + cl;
    const int valid = T.n - col < 4 ? (int)(T.n - col) : 4;
    if (valid <= 0) return;
#pragma unroll
    for (int p = 0; p < kLrBand / 8; ++p) {
        const int rl = rsub + 8 * p;
        const int64_t row = row0 + rl;
        if (row >= T.m) break;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < r; ++c) {  // ascending c
            const float4 q = *reinterpret_cast<const float4*>(qs + c * kLrOutStride + cl);
            const float pv = ps[rl * kLrMaxRank + c];
            g[0] = fmaf(pv, q.x, g[0]);
            g[1] = fmaf(pv, q.y, g[1]);
            g[2] = fmaf(pv, q.z, g[2]);
            g[3] = fmaf(pv, q.w, g[3]);
        }
        const int64_t idx = T.off + row * T.n + col;
        float m[4], b[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
        Vec4<float>::unpack(lr_load4(master + idx, vec, valid), m);
        if (load_mom) Vec4<float>::unpack(lr_load4(mom + idx, vec, valid), b);
        if (resid) {
            // e_k <- M_k - g, M_k from the step's inputs (the rows are overwritten below)
            for (int64_t k = 0; k < K; ++k) {
                float xv[4], ev[4];
                Vec4<float>::unpack(lr_load4(x + k * ld_x + idx, vec, valid), xv);
                Vec4<float>::unpack(lr_load4(resid + k * ld_r + idx, vec, valid), ev);
#pragma unroll
                for (int e = 0; e < 4; ++e) ev[e] = rn_sub(lr_delta(m[e], xv[e], ev[e]), g[e]);
                lr_store4(resid + k * ld_r + idx, vec, valid, Vec4<float>::pack(ev));
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = outer_update_from_g(g[e], m[e], b[e], op);
        lr_store4(master + idx, vec, valid, Vec4<float>::pack(m));
        if (has_mom) lr_store4(mom + idx, vec, valid, Vec4<float>::pack(b));
        const float4 o = Vec4<float>::pack(out);
        for (int64_t k = 0; k < K; ++k) lr_store4(x + k * ld_x + idx, vec, valid, o);
    }
}

static bool lr_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

}  // namespace ga

using namespace ga;

#define GA_LR_COMMON(who)                                                                                       \
    GA_REQUIRE(rank >= 1 && rank <= kLrMaxRank, who ": rank %d is not in 1..%d", rank, kLrMaxRank);             \
    GA_REQUIRE(njobs >= 0 && njobs < (int64_t)INT32_MAX, who ": bad job count %lld", (long long)njobs);

extern "C" GA_API int64_t ga_lowrank_chain(int64_t len, int backproject) {
    if (len < 0) return -1;
    const int unit = backproject ? kLrStep : kLrTile;
    return unit * ceil_div(ceil_div(len, unit), kLrWaves);
}

extern "C" GA_API int ga_lowrank_project(const int32_t* jobs, int64_t njobs, const int64_t* tensors,
                                         const int64_t* segments, const float* x, int64_t K, int64_t ld_x,
                                         const float* master, const float* residual, int64_t ld_r, const float* q,
                                         float q_div, int rank, float* a, hipStream_t stream) {
    clear_error();
    GA_LR_COMMON("ga_lowrank_project")
    GA_REQUIRE(K >= 1, "ga_lowrank_project: K=%lld", (long long)K);
    if (njobs == 0) return GA_OK;
    GA_REQUIRE(jobs && tensors && segments && x && master && q && a, "ga_lowrank_project: null buffer");
    GA_REQUIRE(q_div != 0.0f, "ga_lowrank_project: q_div is 0");
    GA_REQUIRE(lr_aligned(jobs, 16) && lr_aligned(tensors, 8) && lr_aligned(segments, 8),
               "ga_lowrank_project: the job table must be 16-byte, the plan tables 8-byte aligned");
    GA_REQUIRE(lr_aligned(x, 4) && lr_aligned(master, 4) && lr_aligned(residual, 4) && lr_aligned(q, 4) &&
                   lr_aligned(a, 4), "ga_lowrank_project: a buffer is not 4-byte aligned");
    const int aligned = lr_aligned(x, 16) && lr_aligned(master, 16) && lr_aligned(residual, 16) && lr_aligned(a, 16) &&
                        (K == 1 || ld_x % 4 == 0) && (K == 1 || residual == nullptr || ld_r % 4 == 0);
    LrRows R{x, K, ld_x, master, residual, ld_r};
    hipLaunchKernelGGL(lowrank_project_kernel, dim3((unsigned)njobs), dim3(kLrThreads), 0, stream,
                       (const int4*)jobs, tensors, segments, R, q, q_div, rank, aligned, a);
    return check_launch("ga_lowrank_project");
}

extern "C" GA_API int ga_lowrank_orthonormalize(const int64_t* tensors, int64_t ntensors, int rank, float* a,
                                                hipStream_t stream) {
    clear_error();
    GA_REQUIRE(rank >= 1 && rank <= kLrMaxRank, "ga_lowrank_orthonormalize: rank %d is not in 1..%d", rank,
               kLrMaxRank);
    GA_REQUIRE(ntensors >= 0 && ntensors < (int64_t)INT32_MAX, "ga_lowrank_orthonormalize: bad tensor count %lld",
               (long long)ntensors);
    if (ntensors == 0) return GA_OK;
    GA_REQUIRE(tensors && a, "ga_lowrank_orthonormalize: null buffer");
    GA_REQUIRE(lr_aligned(tensors, 8) && lr_aligned(a, 4), "ga_lowrank_orthonormalize: misaligned buffer");
    hipLaunchKernelGGL(lowrank_orth_kernel, dim3((unsigned)ntensors), dim3(kLrOrthThreads), 0, stream, tensors, rank,
                       a);
    return check_launch("ga_lowrank_orthonormalize");
}

extern "C" GA_API int ga_lowrank_backproject(const int32_t* jobs, int64_t njobs, const int64_t* tensors,
                                             const float* x, int64_t K, int64_t ld_x, const float* master,
                                             const float* residual, int64_t ld_r, const float* a, int rank, float* b,
                                             hipStream_t stream) {
    clear_error();
    GA_LR_COMMON("ga_lowrank_backproject")
    GA_REQUIRE(K >= 1, "ga_lowrank_backproject: K=%lld", (long long)K);
    if (njobs == 0) return GA_OK;
    GA_REQUIRE(jobs && tensors && x && master && a && b, "ga_lowrank_backproject: null buffer");
    GA_REQUIRE(lr_aligned(jobs, 16) && lr_aligned(tensors, 8),
               "ga_lowrank_backproject: the job table must be 16-byte, the plan table 8-byte aligned");
    GA_REQUIRE(lr_aligned(x, 4) && lr_aligned(master, 4) && lr_aligned(residual, 4) && lr_aligned(a, 4) &&
                   lr_aligned(b, 4), "ga_lowrank_backproject: a buffer is not 4-byte aligned");
    LrRows R{x, K, ld_x, master, residual, ld_r};
    hipLaunchKernelGGL(lowrank_backproject_kernel, dim3((unsigned)njobs), dim3(kLrThreads), 0, stream,
                       (const int4*)jobs, tensors, R, a, rank, b);
    return check_launch("ga_lowrank_backproject");
}

extern "C" GA_API int ga_diloco_outer_lowrank(const int32_t* jobs, int64_t njobs, const int64_t* tensors,
                                              const int64_t* segments, const float* a, const float* q, float q_div,
                                              int rank, float* x, int64_t K, int64_t ld_x, float* residual,
                                              int64_t ld_r, float divisor, float* master, float* mom, int first_step,
                                              float lr, float momentum, float dampening, float weight_decay,
                                              int nesterov, hipStream_t stream) {
    clear_error();
    GA_LR_COMMON("ga_diloco_outer_lowrank")
    GA_REQUIRE(K >= 1, "ga_diloco_outer_lowrank: K=%lld", (long long)K);
    if (njobs == 0) return GA_OK;
    GA_REQUIRE(jobs && tensors && segments && a && q && x && master, "ga_diloco_outer_lowrank: null buffer");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_lowrank: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(divisor != 0.0f && q_div != 0.0f, "ga_diloco_outer_lowrank: divisor or q_div is 0");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_lowrank: Nesterov momentum requires a momentum and zero dampening");
    GA_REQUIRE(lr_aligned(jobs, 16) && lr_aligned(tensors, 8) && lr_aligned(segments, 8),
               "ga_diloco_outer_lowrank: the job table must be 16-byte, the plan tables 8-byte aligned");
    GA_REQUIRE(lr_aligned(x, 4) && lr_aligned(master, 4) && lr_aligned(residual, 4) && lr_aligned(mom, 4) &&
                   lr_aligned(a, 4) && lr_aligned(q, 4), "ga_diloco_outer_lowrank: a buffer is not 4-byte aligned");
    if (momentum == 0.0f) mom = nullptr;
    const int aligned = lr_aligned(x, 16) && lr_aligned(master, 16) && lr_aligned(residual, 16) &&
                        lr_aligned(mom, 16) && lr_aligned(a, 16) && (K == 1 || ld_x % 4 == 0) &&
                        (K == 1 || residual == nullptr || ld_r % 4 == 0);
    // the divisor of the update is 1: g is formed here, not a sum to be divided
    QuantOuterParams op{1.0f, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    hipLaunchKernelGGL(diloco_outer_lowrank_kernel, dim3((unsigned)njobs), dim3(kLrThreads), 0, stream,
                       (const int4*)jobs, tensors, segments, a, q, q_div, rank, x, K, ld_x, residual, ld_r, master,
                       mom, op, divisor, aligned);
    return check_launch("ga_diloco_outer_lowrank");
}
