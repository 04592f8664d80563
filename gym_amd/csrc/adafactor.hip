// Adafactor inner step on the flat arena: factored second moments (one row vector and one column
// vector per matrix, no first moment) for every tensor of K replica rows, as five launches over job
// tables (torch/optim/_adafactor.py, _single_tensor_adafactor).  Roofline: HBM, 24 bytes per matrix
// element (g three times, p twice and once written); DESIGN.md §3 "Adafactor inner step".
//
// Tables (built once per arena layout and present set on the host, gym_amd/fused_optim.py
// AdafactorPlan): tens, int64 rows {off, rows, cols, matrix, state, rowpart, colpart, job0, njobs, rt,
// ct, psq, usq, scal, 0, 0}, and int32 job rows {tensor, tile row, tile column, 0}, one workgroup each;
// the replica is the grid's second dimension (include/gym_amd.h).  `state` holds row_var [rows] and
// col_var [cols] of a matrix, or the variance of a vector; `work` the partial sums and the scalars
// {alpha, max(mean(row_var), eps1), step, 0} of every tensor.
//
// stats     a 64 x 256 tile, 256 threads: wave w owns rows 16 w .. 16 w + 15 of the tile, a lane 4
//           consecutive columns (one 16-byte load of g and of p per row; cols % 4 != 0 or a base that is
//           not 16-byte aligned: a lane owns columns lane + 64 j, scalar loads).  g (x clip, written
//           back) is squared once: a lane keeps 16 row sums and 4 column sums.  The 16 row sums cross
//           the wave in ONE transposing butterfly (17 exchanges: at distance 32 a lane hands over 8
//           sums and keeps 8, then 4, 2, 1, then two plain steps) instead of 16 butterflies of 6; the
//           column sums cross the waves through LDS, waves ascending.  A vector is cut into chunks of
//           4096 elements, whose variance is updated in place.
// reduce    one workgroup per tensor: partials added in ascending tile order, row_var / col_var lerped,
//           then mean(row_var) and sum p^2 by one fixed tree; alpha.
// unorm     stats' tiling: u = g rsqrt(max(row_var_i col_var_j / mean, eps1^2)), the tile's sum u^2.
// scale     one workgroup per tensor: step = -alpha / max(1, ||u|| / (sqrt(numel) d)).
// apply     unorm's tiling and arithmetic: p = p wd_factor + step u.
//
// Determinism: no atomics, every output element has one owner, every reduction a fixed order.
#include "ga_common.h"
#include "adam_math.h"  // lerp_torch

namespace ga {

constexpr int kAfThreads = 256;
constexpr int kAfFields = 16;
constexpr int kAfTileR = 64;    // tile rows: 16 per wave
constexpr int kAfTileC = 256;   // tile columns: 4 per lane
constexpr int kAfWaveRows = 16;
constexpr int kAfChunk = 4096;  // elements of a vector job: 16 per thread
constexpr int kAfReduce = 1024;  // threads of the per-tensor kernels

struct AfTen {
    int64_t off, rows, cols, matrix, state, rowpart, colpart, job0, njobs, rt, ct, psq, usq, scal;
};
__device__ __forceinline__ AfTen af_ten(const int64_t* tens, int t) {
    const int64_t* p = tens + (int64_t)t * kAfFields;
    return AfTen{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13]};
}

// Sum over the workgroup of kWaves waves, every wave by the same butterfly, the waves ascending;
// every thread returns it.  `red` holds kWaves floats and is free again after the call.
template <int kWaves>
__device__ __forceinline__ float af_block_sum(float v, float* red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();  // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += red[w];
    return s;
}

// Column j of a lane within the tile: 4 consecutive ones (16-byte path) or lane + 64 j.
template <bool kVec>
__device__ __forceinline__ int af_col(int lane, int j) {
    return kVec ? 4 * lane + j : lane + 64 * j;
}

// The lane's 4 elements of a row (row: the row's first element, c0: the tile's first column);
// ok[j]: inside the matrix.  Elements outside read as 0.
template <bool kVec>
__device__ __forceinline__ void af_load(const float* row, int64_t c0, int lane, int64_t cols, float (&v)[4],
                                        bool (&ok)[4]) {
    if (kVec) {
        const int64_t c = c0 + 4 * lane;
        const bool in = c < cols;  // cols % 4 == 0: all four or none
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) t = *reinterpret_cast<const float4*>(row + c);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        ok[0] = ok[1] = ok[2] = ok[3] = in;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t c = c0 + lane + 64 * j;
            ok[j] = c < cols;
            v[j] = ok[j] ? row[c] : 0.f;
        }
    }
}

template <bool kVec>
__device__ __forceinline__ void af_store(float* row, int64_t c0, int lane, const float (&v)[4], const bool (&ok)[4]) {
    if (kVec) {
        if (ok[0]) *reinterpret_cast<float4*>(row + c0 + 4 * lane) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ok[j]) row[c0 + lane + 64 * j] = v[j];
    }
}

// The 16-byte path: rows of 4 n columns whose first element is 16-byte aligned in every buffer given.
__device__ __forceinline__ bool af_vec_ok(int64_t cols, const void* a, const void* b) {
    return (cols & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

// Sum 16 values per lane across the wave: afterwards v[0] of the lanes with (lane & 3) == 0 is the
// wave's sum of value af_fold_index(lane).  At distance d a lane keeps one half of its values (the
// upper half if lane & d) and adds the partner's copy of that half: 8 + 4 + 2 + 1 exchanges, then
// two plain butterfly steps over the four lanes that hold the same value.
__device__ __forceinline__ void af_fold16(float (&v)[16], int lane) {
#pragma unroll
    for (int h = 8, d = 32; h >= 1; h >>= 1, d >>= 1) {
        const bool upper = (lane & d) != 0;
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const float send = upper ? v[j] : v[j + h];
            const float keep = upper ? v[j + h] : v[j];
            v[j] = keep + __shfl_xor(send, d, 64);
        }
    }
    v[0] += __shfl_xor(v[0], 2, 64);
    v[0] += __shfl_xor(v[0], 1, 64);
}
__device__ __forceinline__ int af_fold_index(int lane) {
    return ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
}

template <bool kVec>
__device__ __forceinline__ void af_stats_tile(const AfTen& T, const int4 job, const float* __restrict__ p,
                                              float* __restrict__ g, float* __restrict__ work, float coef, bool scale,
                                              float* colred, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)job.y * kAfTileR + wave * kAfWaveRows, c0 = (int64_t)job.z * kAfTileC;
    float rs[kAfWaveRows], cs[4] = {0.f, 0.f, 0.f, 0.f}, pp = 0.f;
#pragma unroll
    for (int i = 0; i < kAfWaveRows; ++i) {
        rs[i] = 0.f;
        const int64_t r = r0 + i;
        if (r < T.rows) {  // uniform over the wave
            float gv[4], pv[4];
            bool ok[4];
            af_load<kVec>(g + r * T.cols, c0, lane, T.cols, gv, ok);
            af_load<kVec>(p + r * T.cols, c0, lane, T.cols, pv, ok);
            if (scale) {
#pragma unroll
                for (int j = 0; j < 4; ++j) gv[j] *= coef;
                af_store<kVec>(g + r * T.cols, c0, lane, gv, ok);
            }
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float q = gv[j] * gv[j];
                s += q;
                cs[j] += q;
                pp = fmaf(pv[j], pv[j], pp);
            }
            rs[i] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) colred[wave * kAfTileC + af_col<kVec>(lane, j)] = cs[j];
    af_fold16(rs, lane);
    if ((lane & 3) == 0) {
        const int64_t r = r0 + af_fold_index(lane);
        if (r < T.rows) work[T.rowpart + (int64_t)job.z * T.rows + r] = rs[0];
    }
    const float total = af_block_sum<kAfThreads / 64>(pp, red);  // its barriers also complete colred
    if (threadIdx.x == 0) work[T.psq + (blockIdx.x - T.job0)] = total;
    const int64_t c = c0 + threadIdx.x;
    if (c < T.cols) {
        const float* q = colred + threadIdx.x;
        work[T.colpart + (int64_t)job.y * T.cols + c] = ((q[0] + q[kAfTileC]) + q[2 * kAfTileC]) + q[3 * kAfTileC];
    }
}

__global__ __launch_bounds__(kAfThreads) void adafactor_stats_kernel(
    const int4* __restrict__ jobs, const int64_t* __restrict__ tens, const float* __restrict__ param,
    float* __restrict__ grad, float* __restrict__ state, float* __restrict__ work, int64_t ld, int64_t ls,
    int64_t lw, float beta2t, const float* __restrict__ clip_coef) {
    __shared__ float colred[(kAfThreads / 64) * kAfTileC];
    __shared__ float red[kAfThreads / 64];
    const int4 job = jobs[blockIdx.x];
    const AfTen T = af_ten(tens, job.x);
    const int64_t k = blockIdx.y;
    const float coef = clip_coef ? clip_coef[2 * k] : 1.f;
    const bool scale = !(coef >= 1.f);  // a NaN coefficient scales too (ga_sgd_step's rule)
    const float* p = param + k * ld + T.off;
    float* g = grad + k * ld + T.off;
    float* w = work + k * lw;
    if (T.matrix) {
        if (af_vec_ok(T.cols, p, g))
            af_stats_tile<true>(T, job, p, g, w, coef, scale, colred, red);
        else
            af_stats_tile<false>(T, job, p, g, w, coef, scale, colred, red);
        return;
    }
    float* var = state + k * ls + T.state;
    const int64_t n = T.rows * T.cols, base = (int64_t)job.y * kAfChunk + threadIdx.x;
    float pp = 0.f;
#pragma unroll 4
    for (int j = 0; j < kAfChunk / kAfThreads; ++j) {
        const int64_t i = base + (int64_t)kAfThreads * j;
        if (i < n) {
            float gv = g[i];
            if (scale) {
                gv *= coef;
                g[i] = gv;
            }
            var[i] = lerp_torch(var[i], gv * gv, beta2t);
            const float pv = p[i];
            pp = fmaf(pv, pv, pp);
        }
    }
    const float total = af_block_sum<kAfThreads / 64>(pp, red);
    if (threadIdx.x == 0) w[T.psq + (blockIdx.x - T.job0)] = total;
}

__global__ __launch_bounds__(kAfReduce) void adafactor_reduce_kernel(
    const int64_t* __restrict__ tens, float* __restrict__ state, float* __restrict__ work, int64_t ls, int64_t lw,
    float beta2t, float rho, float eps1, float eps2) {
    __shared__ float red[kAfReduce / 64];
    const AfTen T = af_ten(tens, blockIdx.x);
    float* st = state + (int64_t)blockIdx.y * ls + T.state;
    float* w = work + (int64_t)blockIdx.y * lw;
    float rv = 0.f, pp = 0.f;
    if (T.matrix) {
        const float fc = (float)T.cols, fr = (float)T.rows;
        for (int64_t r = threadIdx.x; r < T.rows; r += kAfReduce) {
            float s = 0.f;
            for (int64_t t = 0; t < T.ct; ++t) s += w[T.rowpart + t * T.rows + r];
            const float v = lerp_torch(st[r], s / fc, beta2t);
            st[r] = v;
            rv += v;
        }
        for (int64_t c = threadIdx.x; c < T.cols; c += kAfReduce) {
            float s = 0.f;
            for (int64_t t = 0; t < T.rt; ++t) s += w[T.colpart + t * T.cols + c];
            st[T.rows + c] = lerp_torch(st[T.rows + c], s / fr, beta2t);
        }
    }
    for (int64_t j = threadIdx.x; j < T.njobs; j += kAfReduce) pp += w[T.psq + j];
    rv = af_block_sum<kAfReduce / 64>(rv, red);
    pp = af_block_sum<kAfReduce / 64>(pp, red);
    if (threadIdx.x == 0) {
        const double rms = (double)sqrtf(pp) / sqrt((double)(T.rows * T.cols));
        w[T.scal] = (float)(fmax((double)eps2, rms) * (double)rho);
        w[T.scal + 1] = T.matrix ? fmaxf(rv / (float)T.rows, eps1) : 1.f;
    }
}

// u of the lane's 4 elements of a row: torch's order (product, divide, clamp, rsqrt, multiply).
__device__ __forceinline__ float af_u(float g, float rv, float cv, float denom, float eps1sq) {
    return rsqrtf(fmaxf((rv * cv) / denom, eps1sq)) * g;
}

template <bool kApply, bool kVec>
__device__ __forceinline__ float af_update_tile(const AfTen& T, const int4 job, float* __restrict__ p,
                                                const float* __restrict__ g, const float* __restrict__ st,
                                                const float* __restrict__ work, float eps1sq, float wd_factor) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)job.y * kAfTileR + wave * kAfWaveRows, c0 = (int64_t)job.z * kAfTileC;
    const float denom = work[T.scal + 1], step = kApply ? work[T.scal + 2] : 0.f;
    float cv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + af_col<kVec>(lane, j);
        cv[j] = c < T.cols ? st[T.rows + c] : 0.f;
    }
    float uu = 0.f;
#pragma unroll 4
    for (int i = 0; i < kAfWaveRows; ++i) {
        const int64_t r = r0 + i;
        if (r >= T.rows) break;  // uniform over the wave
        const float rv = st[r];
        float gv[4], pv[4];
        bool ok[4];
        af_load<kVec>(g + r * T.cols, c0, lane, T.cols, gv, ok);
        if (kApply) af_load<kVec>(p + r * T.cols, c0, lane, T.cols, pv, ok);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = ok[j] ? af_u(gv[j], rv, cv[j], denom, eps1sq) : 0.f;
            if (kApply)
                pv[j] = fmaf(step, u, pv[j] * wd_factor);
            else
                uu = fmaf(u, u, uu);
        }
        if (kApply) af_store<kVec>(p + r * T.cols, c0, lane, pv, ok);
    }
    return uu;
}

// unorm (kApply = false: param is not touched, work[usq + job] written) and apply (param written).
template <bool kApply>
__global__ __launch_bounds__(kAfThreads) void adafactor_update_kernel(
    const int4* __restrict__ jobs, const int64_t* __restrict__ tens, float* __restrict__ param,
    const float* __restrict__ grad, const float* __restrict__ state, float* __restrict__ work, int64_t ld,
    int64_t ls, int64_t lw, float eps1sq, float wd_factor) {
    __shared__ float red[kAfThreads / 64];
    const int4 job = jobs[blockIdx.x];
    const AfTen T = af_ten(tens, job.x);
    const int64_t k = blockIdx.y;
    float* p = param + k * ld + T.off;
    const float* g = grad + k * ld + T.off;
    const float* st = state + k * ls + T.state;
    float* w = work + k * lw;
    float uu = 0.f;
    if (T.matrix) {
        if (af_vec_ok(T.cols, kApply ? p : g, g))
            uu = af_update_tile<kApply, true>(T, job, p, g, st, w, eps1sq, wd_factor);
        else
            uu = af_update_tile<kApply, false>(T, job, p, g, st, w, eps1sq, wd_factor);
    } else {
        const int64_t n = T.rows * T.cols, base = (int64_t)job.y * kAfChunk + threadIdx.x;
        const float step = kApply ? w[T.scal + 2] : 0.f;
#pragma unroll 4
        for (int j = 0; j < kAfChunk / kAfThreads; ++j) {
            const int64_t i = base + (int64_t)kAfThreads * j;
            if (i < n) {
                const float u = rsqrtf(fmaxf(st[i], eps1sq)) * g[i];
                if (kApply)
                    p[i] = fmaf(step, u, p[i] * wd_factor);
                else
                    uu = fmaf(u, u, uu);
            }
        }
    }
    if (!kApply) {
        const float total = af_block_sum<kAfThreads / 64>(uu, red);
        if (threadIdx.x == 0) w[T.usq + (blockIdx.x - T.job0)] = total;
    }
}

__global__ __launch_bounds__(kAfReduce) void adafactor_scale_kernel(const int64_t* __restrict__ tens,
                                                                    float* __restrict__ work, int64_t lw, float d) {
    __shared__ float red[kAfReduce / 64];
    const AfTen T = af_ten(tens, blockIdx.x);
    float* w = work + (int64_t)blockIdx.y * lw;
    float uu = 0.f;
    for (int64_t j = threadIdx.x; j < T.njobs; j += kAfReduce) uu += w[T.usq + j];
    uu = af_block_sum<kAfReduce / 64>(uu, red);
    if (threadIdx.x == 0) {
        const double rms = (double)sqrtf(uu) / (sqrt((double)(T.rows * T.cols)) * (double)d);
        w[T.scal + 2] = (float)(-(double)w[T.scal] / fmax(1.0, rms));
    }
}

static bool af_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

}  // namespace ga

using namespace ga;

// The checks every entry shares; `count` jobs or tensors of a launch whose second dimension is K.
#define GA_AF_GRID(who, count)                                                                                  \
    GA_REQUIRE(count >= 0 && count < (int64_t)INT32_MAX, who ": bad table length %lld", (long long)count);     \
    GA_REQUIRE(K >= 1 && K <= 65535, who ": K=%lld is not in 1..65535", (long long)K);                          \
    if (count == 0) return GA_OK;                                                                                \
    GA_REQUIRE(tens && af_aligned(tens, 8), who ": the tensor table is null or not 8-byte aligned");

#define GA_AF_JOBS(who) \
    GA_REQUIRE(jobs && af_aligned(jobs, 16), who ": the job table is null or not 16-byte aligned");

extern "C" GA_API int ga_adafactor_fields(void) { return kAfFields; }

extern "C" GA_API int ga_adafactor_stats(const int32_t* jobs, int64_t njobs, const int64_t* tens, const float* param,
                                         float* grad, float* state, float* work, int64_t K, int64_t ld, int64_t ls,
                                         int64_t lw, float beta2t, const float* clip_coef, hipStream_t stream) {
    clear_error();
    GA_AF_GRID("ga_adafactor_stats", njobs)
    GA_AF_JOBS("ga_adafactor_stats")
    GA_REQUIRE(param && grad && state && work, "ga_adafactor_stats: null buffer");
    GA_REQUIRE(af_aligned(param, 4) && af_aligned(grad, 4) && af_aligned(state, 4) && af_aligned(work, 4) &&
                   af_aligned(clip_coef, 4), "ga_adafactor_stats: misaligned buffer");
    GA_REQUIRE(ld >= 0 && ls >= 0 && lw >= 0, "ga_adafactor_stats: negative row length");
    GA_REQUIRE(beta2t > 0.f && beta2t <= 1.f, "ga_adafactor_stats: beta2t %g is not in (0, 1]", (double)beta2t);
    hipLaunchKernelGGL(adafactor_stats_kernel, dim3((unsigned)njobs, (unsigned)K), dim3(kAfThreads), 0, stream,
                       (const int4*)jobs, tens, param, grad, state, work, ld, ls, lw, beta2t, clip_coef);
    return check_launch("ga_adafactor_stats");
}

extern "C" GA_API int ga_adafactor_reduce(const int64_t* tens, int64_t ntens, float* state, float* work, int64_t K,
                                          int64_t ls, int64_t lw, float beta2t, float rho, float eps1, float eps2,
                                          hipStream_t stream) {
    clear_error();
    GA_AF_GRID("ga_adafactor_reduce", ntens)
    GA_REQUIRE(state && work, "ga_adafactor_reduce: null buffer");
    GA_REQUIRE(af_aligned(state, 4) && af_aligned(work, 4), "ga_adafactor_reduce: misaligned buffer");
    GA_REQUIRE(ls >= 0 && lw >= 0, "ga_adafactor_reduce: negative row length");
    GA_REQUIRE(beta2t > 0.f && beta2t <= 1.f, "ga_adafactor_reduce: beta2t %g is not in (0, 1]", (double)beta2t);
    GA_REQUIRE(rho >= 0.f && eps1 >= 0.f && eps2 >= 0.f, "ga_adafactor_reduce: rho, eps1 and eps2 must be >= 0");
    hipLaunchKernelGGL(adafactor_reduce_kernel, dim3((unsigned)ntens, (unsigned)K), dim3(kAfReduce), 0, stream, tens,
                       state, work, ls, lw, beta2t, rho, eps1, eps2);
    return check_launch("ga_adafactor_reduce");
}

extern "C" GA_API int ga_adafactor_unorm(const int32_t* jobs, int64_t njobs, const int64_t* tens, const float* grad,
                                         const float* state, float* work, int64_t K, int64_t ld, int64_t ls,
                                         int64_t lw, float eps1, hipStream_t stream) {
    clear_error();
    GA_AF_GRID("ga_adafactor_unorm", njobs)
    GA_AF_JOBS("ga_adafactor_unorm")
    GA_REQUIRE(grad && state && work, "ga_adafactor_unorm: null buffer");
    GA_REQUIRE(af_aligned(grad, 4) && af_aligned(state, 4) && af_aligned(work, 4),
               "ga_adafactor_unorm: misaligned buffer");
    GA_REQUIRE(ld >= 0 && ls >= 0 && lw >= 0, "ga_adafactor_unorm: negative row length");
    GA_REQUIRE(eps1 >= 0.f, "ga_adafactor_unorm: eps1 %g is negative", (double)eps1);
    hipLaunchKernelGGL(adafactor_update_kernel<false>, dim3((unsigned)njobs, (unsigned)K), dim3(kAfThreads), 0,
                       stream, (const int4*)jobs, tens, (float*)nullptr, grad, state, work, ld, ls, lw, eps1 * eps1,
                       1.f);
    return check_launch("ga_adafactor_unorm");
}

extern "C" GA_API int ga_adafactor_scale(const int64_t* tens, int64_t ntens, float* work, int64_t K, int64_t lw,
                                         float d, hipStream_t stream) {
    clear_error();
    GA_AF_GRID("ga_adafactor_scale", ntens)
    GA_REQUIRE(work && af_aligned(work, 4), "ga_adafactor_scale: null or misaligned buffer");
    GA_REQUIRE(lw >= 0, "ga_adafactor_scale: negative row length");
    GA_REQUIRE(d >= 1.f, "ga_adafactor_scale: d %g is below 1", (double)d);
    hipLaunchKernelGGL(adafactor_scale_kernel, dim3((unsigned)ntens, (unsigned)K), dim3(kAfReduce), 0, stream, tens,
                       work, lw, d);
    return check_launch("ga_adafactor_scale");
}

extern "C" GA_API int ga_adafactor_apply(const int32_t* jobs, int64_t njobs, const int64_t* tens, float* param,
                                         const float* grad, const float* state, const float* work, int64_t K,
                                         int64_t ld, int64_t ls, int64_t lw, float eps1, float wd_factor,
                                         hipStream_t stream) {
    clear_error();
    GA_AF_GRID("ga_adafactor_apply", njobs)
    GA_AF_JOBS("ga_adafactor_apply")
    GA_REQUIRE(param && grad && state && work, "ga_adafactor_apply: null buffer");
    GA_REQUIRE(af_aligned(param, 4) && af_aligned(grad, 4) && af_aligned(state, 4) && af_aligned(work, 4),
               "ga_adafactor_apply: misaligned buffer");
    GA_REQUIRE(ld >= 0 && ls >= 0 && lw >= 0, "ga_adafactor_apply: negative row length");
    GA_REQUIRE(eps1 >= 0.f, "ga_adafactor_apply: eps1 %g is negative", (double)eps1);
    hipLaunchKernelGGL(adafactor_update_kernel<true>, dim3((unsigned)njobs, (unsigned)K), dim3(kAfThreads), 0, stream,
                       (const int4*)jobs, tens, param, grad, state, const_cast<float*>(work), ld, ls, lw, eps1 * eps1,
                       wd_factor);
    return check_launch("ga_adafactor_apply");
}
