// 8-bit AdamW inner step on the flat arena: both moments kept as 8-bit codes of a
// non-uniform "dynamic" code book under one fp32 scale per 64-element block (Dettmers et
// al., "8-bit Optimizers via Block-wise Quantization"), de-quantised, updated in fp32 by
// adam_elem and re-quantised inside one streaming pass.  2.125 B of state per element
// instead of 8, and 16.25 B moved per element (p read and written, g read, two code bytes
// read and written, two scales per 64 elements read and written) against ga_adam_step's 28.
//
// Work split: a lane owns 4 consecutive elements (a float4 of p, a float4 of g, one 4-byte
// word of each code array), so a 64-element block is 16 lanes = one DPP row, a wavefront
// does four blocks per iteration and a workgroup of four waves 1024 elements.  The grid is
// persistent (kGrid workgroups over all replicas, the replica on grid.y) and strides over
// the row, so the tables below are loaded once per workgroup and used for many iterations.
//
// Block maxima: |m| and v are reduced over the 16 lanes of a row with four row-local DPP
// steps (two quad permutes, row_half_mirror, row_mirror), a butterfly that leaves the
// maximum in every lane of the row.  No LDS, no traffic between rows, no atomics.
//
// Tables (the caller's: gym_amd.ops.adam8_tables is their only definition) sit in LDS, 4 KB
// per workgroup.  Decode is one read of codes[row][q].  Encode counts the thresholds below
// x / absmax with a branch-free 8-step search.  The 255 sorted thresholds of a row are laid
// out in LDS as an implicit search tree in breadth-first order (node i has children 2i and
// 2i + 1): the lanes of a wave then read, at step k, among 2^k CONSECUTIVE words, which are
// in different banks up to step 5, where the sorted order would put every probe of the
// first three steps in one bank (index = 31 mod 32) and the next two steps in two and four.
// The leaf reached is the count.
#include "ga_common.h"
#include "adam_math.h"

namespace ga {

constexpr int kA8Block = 256;             // four waves
constexpr int kA8Iter = kA8Block * 4;     // elements of a workgroup iteration
constexpr int kA8QB = 64;                 // elements under one scale
constexpr int kA8Grid = 2048;             // persistent workgroups over all replicas (8 per CU)

// a * b as one rounded product that the compiler must not contract into a following add or
// subtract: hipcc contracts across statements by default, and HIP's __fmul_rn is a plain
// product to it (with it the ISA had the decode product inside g - m as an fma)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// max over the row's lanes of x and its DPP partner
template <int kCtrl>
__device__ __forceinline__ float dpp_max(float x) {
    const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xf, 0xf, false);
    return fmaxf(x, __int_as_float(y));
}

// The maximum of x (>= 0) over the 16 lanes of a DPP row, in every lane of the row.  The
// rows of a wave are all in the loop or all out of it (n % 64 == 0), so every partner is live.
__device__ __forceinline__ float row_max(float x) {
    x = dpp_max<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x = dpp_max<0x4E>(x);   // quad_perm [2, 3, 0, 1]
    x = dpp_max<0x141>(x);  // row_half_mirror: lane i <-> 7 - i of its half row
    return dpp_max<0x140>(x);  // row_mirror: lane i <-> 15 - i
}

struct A8Tables {
    float code[2][256];  // code books: row 0 signed (exp_avg), row 1 unsigned (exp_avg_sq)
    float tree[2][256];  // thresholds as search trees: node 1 the root, [0] unused
};

// codes: [2, 256] or null (encode only needs the thresholds); thresholds: [2, 256], 255 used
__device__ __forceinline__ void load_tables(A8Tables& T, const float* __restrict__ codes,
                                            const float* __restrict__ thresholds) {
    for (int i = threadIdx.x; i < 512; i += kA8Block) {
        const int r = i >> 8, node = i & 255;
        if (codes) T.code[r][node] = codes[i];
        float t = 0.f;
        if (node) {  // node = 2^k + j is the (2j + 1) * 2^(7 - k) - th smallest threshold
            const int k = 31 - __clz(node), j = node - (1 << k);
            t = thresholds[r * 256 + (((2 * j + 1) << (7 - k)) - 1)];
        }
        T.tree[r][node] = t;
    }
    __syncthreads();
}

// number of the row's 255 thresholds that are < x (ties to the lower code)
__device__ __forceinline__ uint32_t search(const float* __restrict__ tree, float x) {
    uint32_t i = 1;
#pragma unroll
    for (int l = 0; l < 8; ++l) i = 2 * i + (tree[i] < x ? 1u : 0u);
    return i & 255u;
}

// The 4 codes of a lane (packed, element 0 in the low byte) and the block's scale: absmax
// over the row, x / absmax as an IEEE division (0 in an all-zero block), the search.
// kUnsigned: a value > 0 whose code comes out 0 is stored as code 1, so a small second
// moment beside a large one rounds the denominator up and never to zero.
template <bool kUnsigned>
__device__ __forceinline__ uint32_t quantise4(const float (&x)[4], const float* __restrict__ tree, float& absmax) {
    absmax = row_max(fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3]))));
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xh = absmax == 0.f ? 0.f : x[e] / absmax;
        uint32_t q = search(tree, xh);
        if (kUnsigned && q == 0 && x[e] > 0.f) q = 1;
        word |= q << (8 * e);
    }
    return word;
}

__device__ __forceinline__ uint32_t load_word(const uint8_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
}
__device__ __forceinline__ void store_word(uint8_t* p, uint32_t w) {
    __builtin_nontemporal_store(w, reinterpret_cast<uint32_t*>(p));
}

__global__ __launch_bounds__(kA8Block) void adam8_step_kernel(
    float* __restrict__ param, float* __restrict__ grad, uint8_t* __restrict__ m_code, float* __restrict__ m_absmax,
    uint8_t* __restrict__ v_code, float* __restrict__ v_absmax, int64_t n, int64_t ld,
    const float* __restrict__ codes, const float* __restrict__ thresholds, AdamParams ap,
    const float* __restrict__ clip_coef) {
    __shared__ A8Tables T;
    load_tables(T, codes, thresholds);
    const int64_t rep = blockIdx.y;
    param += rep * ld;
    grad += rep * ld;
    m_code += rep * ld;
    v_code += rep * ld;
    m_absmax += rep * (ld / kA8QB);
    v_absmax += rep * (ld / kA8QB);
    const float coef = clip_coef ? clip_coef[2 * rep] : 1.f;
    const bool scale = !(coef >= 1.f);  // a NaN coefficient scales too (ga_adam_step's rule)
    for (int64_t lo = (int64_t)blockIdx.x * kA8Iter; lo < n; lo += (int64_t)gridDim.x * kA8Iter) {
        const int64_t at = lo + 4 * (int64_t)threadIdx.x;  // this lane's first element
        if (at >= n) continue;
        const int64_t blk = at / kA8QB;
        float pp[4], gg[4], mm[4], vv[4];
        Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(param + at)), pp);
        Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(grad + at)), gg);
        const uint32_t mw = load_word(m_code + at), vw = load_word(v_code + at);
        const float ma = m_absmax[blk], va = v_absmax[blk];
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // rounded products: the decoded m feeds g - m, which must not become an fma
            mm[e] = mul_rn(T.code[0][(mw >> (8 * e)) & 255u], ma);
            vv[e] = mul_rn(T.code[1][(vw >> (8 * e)) & 255u], va);
        }
        if (scale) {
#pragma unroll
            for (int e = 0; e < 4; ++e) gg[e] = mul_rn(gg[e], coef);
            stream_store(reinterpret_cast<float4*>(grad + at), Vec4<float>::pack(gg));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) adam_elem(pp[e], gg[e], mm[e], vv[e], ap);  // p from the fresh fp32 m and v
        store_sc1(reinterpret_cast<float4*>(param + lo), threadIdx.x, Vec4<float>::pack(pp));
        float new_ma, new_va;
        store_word(m_code + at, quantise4<false>(mm, T.tree[0], new_ma));
        store_word(v_code + at, quantise4<true>(vv, T.tree[1], new_va));
        if ((threadIdx.x & 15) == 0) {
            m_absmax[blk] = new_ma;
            v_absmax[blk] = new_va;
        }
    }
}

template <bool kUnsigned>
__global__ __launch_bounds__(kA8Block) void adam8_encode_kernel(const float* __restrict__ x, uint8_t* __restrict__ code,
                                                                float* __restrict__ absmax, int64_t n, int64_t ld,
                                                                const float* __restrict__ thresholds) {
    __shared__ A8Tables T;
    load_tables(T, nullptr, thresholds);
    const int64_t rep = blockIdx.y;
    x += rep * ld;
    code += rep * ld;
    absmax += rep * (ld / kA8QB);
    for (int64_t lo = (int64_t)blockIdx.x * kA8Iter; lo < n; lo += (int64_t)gridDim.x * kA8Iter) {
        const int64_t at = lo + 4 * (int64_t)threadIdx.x;
        if (at >= n) continue;
        float xx[4], am;
        Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(x + at)), xx);
        store_word(code + at, quantise4<kUnsigned>(xx, T.tree[kUnsigned], am));
        if ((threadIdx.x & 15) == 0) absmax[at / kA8QB] = am;
    }
}

}  // namespace ga

using namespace ga;

// What both entries require of their sizes, in the entry's name; *grid = workgroups per
// replica, 0 when there is nothing to do (n == 0).
static int a8_grid(const char* who, int64_t n, int64_t K, int64_t ld, int64_t* grid) {
    *grid = 0;
    GA_REQUIRE(n >= 0 && K >= 1 && K <= 65535, "%s: bad sizes n=%lld K=%lld", who, (long long)n, (long long)K);
    if (n == 0) return GA_OK;
    GA_REQUIRE(n % kA8QB == 0, "%s: n must be a multiple of 64 (whole blocks), got %lld", who, (long long)n);
    GA_REQUIRE(ld % kA8QB == 0 && ld >= n, "%s: ld must be >= n and a multiple of 64, got %lld", who, (long long)ld);
    const int64_t want = ceil_div(n, kA8Iter), cap = kA8Grid / K > 1 ? kA8Grid / K : 1;
    *grid = want < cap ? want : cap;
    return GA_OK;
}

extern "C" GA_API int ga_adam8_step(int dtype, void* param, void* grad, uint8_t* exp_avg_code, float* exp_avg_absmax,
                                    uint8_t* exp_avg_sq_code, float* exp_avg_sq_absmax, int64_t K, int64_t ld,
                                    int64_t n, const float* codes, const float* thresholds, float lerp_w, float beta2,
                                    float one_m_beta2, float eps, float wd_factor, float l2_wd, float step_size,
                                    float bc2_sqrt, const float* clip_coef, hipStream_t stream) {
    clear_error();
    int64_t grid;
    if (int e = a8_grid("ga_adam8_step", n, K, ld, &grid)) return e;
    if (grid == 0) return GA_OK;
    GA_REQUIRE(param && grad && exp_avg_code && exp_avg_absmax && exp_avg_sq_code && exp_avg_sq_absmax && codes &&
                   thresholds,
               "ga_adam8_step: null buffer");
    GA_REQUIRE(dtype == GA_F32, "ga_adam8_step: only float32 arenas are fused (dtype %d)", dtype);
    GA_REQUIRE(((uintptr_t)param | (uintptr_t)grad) % 16 == 0, "ga_adam8_step: param and grad must be 16-byte aligned");
    GA_REQUIRE(((uintptr_t)exp_avg_code | (uintptr_t)exp_avg_sq_code | (uintptr_t)exp_avg_absmax |
                (uintptr_t)exp_avg_sq_absmax | (uintptr_t)codes | (uintptr_t)thresholds) % 4 == 0,
               "ga_adam8_step: codes, scales and tables must be 4-byte aligned");
    GA_REQUIRE(bc2_sqrt > 0.f, "ga_adam8_step: bc2_sqrt must be > 0");
    const AdamParams ap{lerp_w, beta2, one_m_beta2, eps, wd_factor, l2_wd, step_size, bc2_sqrt};
    hipLaunchKernelGGL(adam8_step_kernel, dim3((unsigned)grid, (unsigned)K), dim3(kA8Block), 0, stream, (float*)param,
                       (float*)grad, exp_avg_code, exp_avg_absmax, exp_avg_sq_code, exp_avg_sq_absmax, n, ld, codes,
                       thresholds, ap, clip_coef);
    return check_launch("ga_adam8_step");
}

extern "C" GA_API int ga_adam8_encode(const float* x, uint8_t* code, float* absmax, int64_t K, int64_t ld, int64_t n,
                                      int row, const float* thresholds, hipStream_t stream) {
    clear_error();
    int64_t grid;
    if (int e = a8_grid("ga_adam8_encode", n, K, ld, &grid)) return e;
    if (grid == 0) return GA_OK;
    GA_REQUIRE(x && code && absmax && thresholds, "ga_adam8_encode: null buffer");
    GA_REQUIRE(row == 0 || row == 1, "ga_adam8_encode: row must be 0 (signed) or 1 (unsigned), got %d", row);
    GA_REQUIRE((uintptr_t)x % 16 == 0, "ga_adam8_encode: x must be 16-byte aligned");
    GA_REQUIRE(((uintptr_t)code | (uintptr_t)absmax | (uintptr_t)thresholds) % 4 == 0,
               "ga_adam8_encode: codes, scales and tables must be 4-byte aligned");
    const dim3 g((unsigned)grid, (unsigned)K);
    if (row)
        hipLaunchKernelGGL(adam8_encode_kernel<true>, g, dim3(kA8Block), 0, stream, x, code, absmax, n, ld, thresholds);
    else
        hipLaunchKernelGGL(adam8_encode_kernel<false>, g, dim3(kA8Block), 0, stream, x, code, absmax, n, ld,
                           thresholds);
    return check_launch("ga_adam8_encode");
}
