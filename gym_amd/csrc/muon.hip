// Muon inner step on the flat arena: momentum + Newton-Schulz orthogonalisation of every
// hidden matrix of a replica row as grouped launches over job tables (torch.optim.Muon:
// torch/optim/_muon.py).  Roofline: the bf16 MFMA for the three products of an iteration,
// HBM for prepare and apply (DESIGN.md §3 "Muon inner step").
//
// Tables (built once per arena layout on the host, gym_amd/fused_optim.py MuonPlan): mats, int64
// rows {off, rows, cols, m_pad, n_pad, x, xt0, xt1, a, b, tall, job0, njobs, ratio, 0, 0}, and
// int32 job rows {matrix, tile row, tile column, 0}, one workgroup each (include/gym_amd.h).
// The bf16 workspace holds per matrix X (m_pad x n_pad, updated in place), X^T in two ping-pong
// copies (n_pad x m_pad) and A, B (m_pad x m_pad), zero beyond m x n.  The products read and write
// whole tiles, padding included: zero rows and columns of X give zero rows and columns of A, B and
// B X, so for finite inputs the padding is rewritten with exact zeros and there is no edge code.
//
// prepare   job = a 64 x 64 tile of the parameter's own rows x cols: g (x clip), buf <- lerp,
//           u, bf16(u) stored as it lies into the buffer of the parameter's orientation (X, or
//           X^T copy 0 of a tall matrix) and through an LDS image transposed into the other;
//           the tile's sum of bf16(u)^2 goes to partials[job] (wave butterfly, waves ascending).
// scale     one wave per matrix: s = 1 / max(sqrt(sum of its partials), eps).  X is never
//           divided: the first iteration carries s in its scalars (A = s^2 U U^T, X' = a s U +
//           s B U), so the workspace is written once per product and bf16(u) is rounded once.
// gemm      C = alpha D + beta L R^T, every product of the iteration in this one "NT" form (A and
//           B are symmetric): each lane's MFMA fragment is 8 consecutive k of a row, 16 bytes.
//           256 threads, macro tile T = 128 (64 for matrices of m_pad = 64): four waves of
//           (T/2)^2, k-step 64 through two LDS buffers filled by 16-byte global loads that are
//           issued before the step's MFMAs and stored after them (one barrier per step), rows
//           padded to 72 bf16 so the 16-byte fragment reads of 8 rows cover all 32 banks.
//           The update needs X with k along its rows, so X^T is kept beside X: the epilogue
//           stores the tile to X and, four consecutive rows of a lane as one 8-byte store, to
//           the other X^T copy; gram and poly use the same store for the mirror tile and so
//           compute only tiles with column >= row.
// apply     job = prepare's tiles: p = p wd_factor - lr ratio s O, O read in the parameter's
//           orientation (no transposition).
//
// Determinism: no atomics, every output element has one owner, every reduction a fixed order.
#include "ga_common.h"
#include "adam_math.h"  // lerp_torch

namespace ga {

constexpr int kMuThreads = 256;
constexpr int kMuFields = 16;
constexpr int kMuPrep = 64;           // prepare / apply tile edge
constexpr int kMuPrepStride = 66;     // LDS image row stride (bf16): 33 dwords, transposed reads conflict-free
constexpr int kMuKStep = 64;          // k per LDS stage
constexpr int kMuStride = kMuKStep + 8;  // LDS row stride (bf16) of the operand tiles: 144 bytes

typedef float mu_f16v __attribute__((ext_vector_type(16)));
typedef __bf16 mu_bf8v __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint16_t mu_f2bf(float f) {  // round to nearest even; NaN stays NaN
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float mu_bf2f(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

struct MuMat {
    int64_t off, rows, cols, m_pad, n_pad, x, xt0, xt1, a, b, tall, job0, njobs;
    float ratio;
    __device__ __forceinline__ int64_t xt(int copy) const { return copy ? xt1 : xt0; }
};
__device__ __forceinline__ MuMat mu_mat(const int64_t* mats, int t) {
    const int64_t* p = mats + (int64_t)t * kMuFields;
    return MuMat{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12],
                 __uint_as_float((uint32_t)p[13])};
}

// Sum over the workgroup, every wave by the same butterfly, the waves ascending; thread 0 holds it.
__device__ __forceinline__ float mu_block_sum(float v, float* red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kMuThreads) void muon_prepare_kernel(
    const int4* __restrict__ jobs, const int64_t* __restrict__ mats, float* __restrict__ grad,
    float* __restrict__ buf, uint16_t* __restrict__ ws, float* __restrict__ partials, float momentum,
    float one_m_momentum, int nesterov, const float* __restrict__ clip_coef) {
    __shared__ uint16_t img[kMuPrep * kMuPrepStride];
    __shared__ float red[kMuThreads / 64];
    const int4 job = jobs[blockIdx.x];
    const MuMat M = mu_mat(mats, job.x);
    const float coef = clip_coef ? clip_coef[0] : 1.f;
    const bool scale = !(coef >= 1.f);  // a NaN coefficient scales too (ga_adam_step's rule)
    // the buffer that has the parameter's orientation, and the other one
    uint16_t* S = ws + (M.tall ? M.xt0 : M.x);
    uint16_t* O = ws + (M.tall ? M.x : M.xt0);
    const int64_t ldS = M.tall ? M.m_pad : M.n_pad, ldO = M.tall ? M.n_pad : M.m_pad;
    const int64_t r0 = (int64_t)job.y * kMuPrep, c0 = (int64_t)job.z * kMuPrep;
    const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6;
    float ss = 0.f;
#pragma unroll 4
    for (int i = 0; i < kMuPrep / 4; ++i) {
        const int rl = lr + 4 * i;
        const int64_t r = r0 + rl, c = c0 + lc;
        uint16_t h = 0;
        if (r < M.rows && c < M.cols) {
            const int64_t idx = M.off + r * M.cols + c;
            float g = grad[idx];
            if (scale) {
                g *= coef;
                grad[idx] = g;
            }
            const float b = lerp_torch(buf[idx], g, one_m_momentum);
            buf[idx] = b;
            const float u = nesterov ? lerp_torch(g, b, momentum) : b;
            h = mu_f2bf(u);
            S[r * ldS + c] = h;
            const float v = mu_bf2f(h);
            ss = fmaf(v, v, ss);
        }
        img[rl * kMuPrepStride + lc] = h;
    }
    const float total = mu_block_sum(ss, red);  // its barrier also completes the image
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
#pragma unroll 4
    for (int i = 0; i < kMuPrep / 4; ++i) {
        const int cl = lr + 4 * i;  // lanes run along the parameter's rows: contiguous in O
        const int64_t r = r0 + lc, c = c0 + cl;
        if (r < M.rows && c < M.cols) O[c * ldO + r] = img[lc * kMuPrepStride + cl];
    }
}

__global__ __launch_bounds__(64) void muon_scale_kernel(const int64_t* __restrict__ mats,
                                                        const float* __restrict__ partials, float eps,
                                                        float* __restrict__ scale) {
    const MuMat M = mu_mat(mats, blockIdx.x);
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < M.njobs; i += 64) acc += partials[M.job0 + i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if (threadIdx.x == 0) scale[blockIdx.x] = 1.f / fmaxf(sqrtf(acc), eps);
}

__global__ __launch_bounds__(kMuThreads) void muon_apply_kernel(
    const int4* __restrict__ jobs, const int64_t* __restrict__ mats, float* __restrict__ param,
    const uint16_t* __restrict__ ws, int parity, const float* __restrict__ scale, float lr, float wd_factor) {
    const int4 job = jobs[blockIdx.x];
    const MuMat M = mu_mat(mats, job.x);
    const uint16_t* S = ws + (M.tall ? M.xt(parity) : M.x);
    const int64_t ldS = M.tall ? M.m_pad : M.n_pad;
    const float step = -(lr * M.ratio) * (scale ? scale[job.x] : 1.f);
    const int64_t r0 = (int64_t)job.y * kMuPrep, c = (int64_t)job.z * kMuPrep + (threadIdx.x & 63);
    if (c >= M.cols) return;
#pragma unroll 4
    for (int i = 0; i < kMuPrep / 4; ++i) {
        const int64_t r = r0 + (threadIdx.x >> 6) + 4 * i;
        if (r >= M.rows) break;
        const int64_t idx = M.off + r * M.cols + c;
        param[idx] = fmaf(step, mu_bf2f(S[r * ldS + c]), param[idx] * wd_factor);
    }
}

// The operands of a product: C (ldc) and its transposed copy CT (ldct, null: none) = alpha D + beta L R^T,
// L and R with Kd columns.
struct MuGemm {
    const uint16_t *L, *R, *D;
    uint16_t *C, *CT;
    int64_t ldl, ldr, ldd, ldc, ldct, Kd;
    float alpha, beta;
};

__device__ __forceinline__ MuGemm mu_operands(const MuMat& M, uint16_t* ws, int kind, int parity, float alpha,
                                              float beta, float s, bool diagonal) {
    MuGemm G;
    if (kind == 0) {  // A = beta s^2 X X^T
        G.L = G.R = ws + M.x;
        G.ldl = G.ldr = M.n_pad;
        G.Kd = M.n_pad;
        G.D = nullptr;
        G.ldd = 0;
        G.C = ws + M.a;
        G.ldc = G.ldct = M.m_pad;
        G.CT = diagonal ? nullptr : G.C;
        G.alpha = 0.f;
        G.beta = beta * s * s;
    } else if (kind == 1) {  // B = alpha A + beta A A^T
        G.L = G.R = G.D = ws + M.a;
        G.ldl = G.ldr = G.ldd = M.m_pad;
        G.Kd = M.m_pad;
        G.C = ws + M.b;
        G.ldc = G.ldct = M.m_pad;
        G.CT = diagonal ? nullptr : G.C;
        G.alpha = alpha;
        G.beta = beta;
    } else {  // X = alpha s X + beta s B (X^T)^T, and its transpose into the other X^T copy
        G.L = ws + M.b;
        G.ldl = M.m_pad;
        G.R = ws + M.xt(parity);
        G.ldr = M.m_pad;
        G.Kd = M.m_pad;
        G.D = ws + M.x;
        G.C = ws + M.x;
        G.ldd = G.ldc = M.n_pad;
        G.CT = ws + M.xt(parity ^ 1);
        G.ldct = M.m_pad;
        G.alpha = alpha * s;
        G.beta = beta * s;
    }
    return G;
}

template <int T>
__global__ __launch_bounds__(kMuThreads) void muon_gemm_kernel(const int4* __restrict__ jobs,
                                                               const int64_t* __restrict__ mats, uint16_t* ws,
                                                               int kind, int parity, float alpha, float beta,
                                                               const float* __restrict__ scale) {
    constexpr int W = T / 2;     // a wave's tile edge
    constexpr int NT = W / 32;   // MFMA tiles per wave and dimension
    constexpr int CH = T / 32;   // 16-byte chunks per thread, operand and k-step (T rows x 8 chunks / 256)
    __shared__ __attribute__((aligned(16))) uint16_t Ls[2][T * kMuStride];
    __shared__ __attribute__((aligned(16))) uint16_t Rs[2][T * kMuStride];
    const int4 job = jobs[blockIdx.x];
    const MuMat M = mu_mat(mats, job.x);
    const MuGemm G = mu_operands(M, ws, kind, parity, alpha, beta, scale ? scale[job.x] : 1.f, job.y == job.z);
    const int64_t row0 = (int64_t)job.y * T, col0 = (int64_t)job.z * T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = (wave >> 1) * W, wc = (wave & 1) * W;
    const int li = lane & 31, lh = lane >> 5;

    // chunk q of this thread: row (tid + 256 q) >> 3 of the tile, k chunk (tid + 256 q) & 7
    const uint16_t* gl[CH];
    const uint16_t* gr[CH];
    int so[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        const int c = threadIdx.x + kMuThreads * q, row = c >> 3, kc = c & 7;
        gl[q] = G.L + (row0 + row) * G.ldl + 8 * kc;
        gr[q] = G.R + (col0 + row) * G.ldr + 8 * kc;
        so[q] = row * kMuStride + 8 * kc;
    }
    uint4 pl[CH], pr[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        pl[q] = *reinterpret_cast<const uint4*>(gl[q]);
        pr[q] = *reinterpret_cast<const uint4*>(gr[q]);
    }
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        *reinterpret_cast<uint4*>(&Ls[0][so[q]]) = pl[q];
        *reinterpret_cast<uint4*>(&Rs[0][so[q]]) = pr[q];
    }
    __syncthreads();

    mu_f16v acc[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nk = (int)(G.Kd / kMuKStep);
    for (int ks = 0; ks < nk; ++ks) {
        const int cur = ks & 1;
        // the next step's operands (the last step loads itself again: staging that is conditional
        // is kept in scratch memory by the compiler)
        const int64_t k0 = (int64_t)(ks + 1 < nk ? ks + 1 : ks) * kMuKStep;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            pl[q] = *reinterpret_cast<const uint4*>(gl[q] + k0);
            pr[q] = *reinterpret_cast<const uint4*>(gr[q] + k0);
        }
        const uint16_t* la = &Ls[cur][(wr + li) * kMuStride + 8 * lh];
        const uint16_t* rb = &Rs[cur][(wc + li) * kMuStride + 8 * lh];
#pragma unroll
        for (int kk = 0; kk < kMuKStep / 16; ++kk) {
            mu_bf8v a[NT], b[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                a[i] = __builtin_bit_cast(mu_bf8v, *reinterpret_cast<const uint4*>(la + 32 * i * kMuStride + 16 * kk));
                b[i] = __builtin_bit_cast(mu_bf8v, *reinterpret_cast<const uint4*>(rb + 32 * i * kMuStride + 16 * kk));
            }
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            *reinterpret_cast<uint4*>(&Ls[cur ^ 1][so[q]]) = pl[q];
            *reinterpret_cast<uint4*>(&Rs[cur ^ 1][so[q]]) = pr[q];
        }
        __syncthreads();
    }

    // register e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of the MFMA tile
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int64_t col = col0 + wc + 32 * j + li;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t rb0 = row0 + wr + 32 * i + 8 * q + 4 * lh;
                uint16_t o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = G.beta * acc[i][j][4 * q + r];
                    if (G.D) v = fmaf(G.alpha, mu_bf2f(G.D[(rb0 + r) * G.ldd + col]), v);
                    o[r] = mu_f2bf(v);
                    G.C[(rb0 + r) * G.ldc + col] = o[r];
                }
                if (G.CT) {
                    uint2 w;
                    w.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
                    w.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
                    *reinterpret_cast<uint2*>(G.CT + col * G.ldct + rb0) = w;
                }
            }
        }
    }
}

static bool mu_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

}  // namespace ga

using namespace ga;

#define GA_MU_JOBS(who)                                                                                   \
    GA_REQUIRE(njobs >= 0 && njobs < (int64_t)INT32_MAX, who ": bad job count %lld", (long long)njobs); \
    if (njobs == 0) return GA_OK;                                                                         \
    GA_REQUIRE(mu_aligned(jobs, 16) && mu_aligned(mats, 8),                                               \
               who ": the job table must be 16-byte, the matrix table 8-byte aligned");

extern "C" GA_API int ga_muon_fields(void) { return kMuFields; }

extern "C" GA_API int ga_muon_prepare(const int32_t* jobs, int64_t njobs, const int64_t* mats, float* grad,
                                      float* buf, void* workspace, float* partials, float momentum,
                                      float one_m_momentum, int nesterov, const float* clip_coef,
                                      hipStream_t stream) {
    clear_error();
    GA_MU_JOBS("ga_muon_prepare")
    GA_REQUIRE(jobs && mats && grad && buf && workspace && partials, "ga_muon_prepare: null buffer");
    GA_REQUIRE(mu_aligned(grad, 4) && mu_aligned(buf, 4) && mu_aligned(partials, 4) && mu_aligned(clip_coef, 4) &&
                   mu_aligned(workspace, 16), "ga_muon_prepare: misaligned buffer (workspace: 16 bytes)");
    GA_REQUIRE(momentum >= 0.f && momentum < 1.f, "ga_muon_prepare: momentum %g is not in [0, 1)", (double)momentum);
    hipLaunchKernelGGL(muon_prepare_kernel, dim3((unsigned)njobs), dim3(kMuThreads), 0, stream, (const int4*)jobs,
                       mats, grad, buf, (uint16_t*)workspace, partials, momentum, one_m_momentum, nesterov ? 1 : 0,
                       clip_coef);
    return check_launch("ga_muon_prepare");
}

extern "C" GA_API int ga_muon_scale(const int64_t* mats, int64_t nmats, const float* partials, float eps,
                                    float* scale, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(nmats >= 0 && nmats < (int64_t)INT32_MAX, "ga_muon_scale: bad matrix count %lld", (long long)nmats);
    if (nmats == 0) return GA_OK;
    GA_REQUIRE(mats && partials && scale, "ga_muon_scale: null buffer");
    GA_REQUIRE(mu_aligned(mats, 8) && mu_aligned(partials, 4) && mu_aligned(scale, 4),
               "ga_muon_scale: misaligned buffer");
    GA_REQUIRE(eps >= 0.f, "ga_muon_scale: eps %g is negative", (double)eps);
    hipLaunchKernelGGL(muon_scale_kernel, dim3((unsigned)nmats), dim3(64), 0, stream, mats, partials, eps, scale);
    return check_launch("ga_muon_scale");
}

extern "C" GA_API int ga_muon_gemm(int kind, int tile, const int32_t* jobs, int64_t njobs, const int64_t* mats,
                                   void* workspace, int parity, float alpha, float beta, const float* scale,
                                   hipStream_t stream) {
    clear_error();
    GA_REQUIRE(kind >= 0 && kind <= 2, "ga_muon_gemm: kind %d is not 0 (gram), 1 (poly) or 2 (update)", kind);
    GA_REQUIRE(tile == 64 || tile == 128, "ga_muon_gemm: tile %d is not 64 or 128", tile);
    GA_REQUIRE(parity == 0 || parity == 1, "ga_muon_gemm: parity %d is not 0 or 1", parity);
    GA_MU_JOBS("ga_muon_gemm")
    GA_REQUIRE(jobs && mats && workspace, "ga_muon_gemm: null buffer");
    GA_REQUIRE(mu_aligned(workspace, 16) && mu_aligned(scale, 4),
               "ga_muon_gemm: misaligned buffer (workspace: 16 bytes)");
    if (tile == 128)
        hipLaunchKernelGGL(muon_gemm_kernel<128>, dim3((unsigned)njobs), dim3(kMuThreads), 0, stream,
                           (const int4*)jobs, mats, (uint16_t*)workspace, kind, parity, alpha, beta, scale);
    else
        hipLaunchKernelGGL(muon_gemm_kernel<64>, dim3((unsigned)njobs), dim3(kMuThreads), 0, stream,
                           (const int4*)jobs, mats, (uint16_t*)workspace, kind, parity, alpha, beta, scale);
    return check_launch("ga_muon_gemm");
}

extern "C" GA_API int ga_muon_apply(const int32_t* jobs, int64_t njobs, const int64_t* mats, float* param,
                                    const void* workspace, int parity, const float* scale, float lr, float wd_factor,
                                    hipStream_t stream) {
    clear_error();
    GA_REQUIRE(parity == 0 || parity == 1, "ga_muon_apply: parity %d is not 0 or 1", parity);
    GA_MU_JOBS("ga_muon_apply")
    GA_REQUIRE(jobs && mats && param && workspace, "ga_muon_apply: null buffer");
    GA_REQUIRE(mu_aligned(param, 4) && mu_aligned(workspace, 16) && mu_aligned(scale, 4),
               "ga_muon_apply: misaligned buffer (workspace: 16 bytes)");
    hipLaunchKernelGGL(muon_apply_kernel, dim3((unsigned)njobs), dim3(kMuThreads), 0, stream, (const int4*)jobs, mats,
                       param, (const uint16_t*)workspace, parity, scale, lr, wd_factor);
    return check_launch("ga_muon_apply");
}
