// Hadamard-rotated int8 / int4 DiLoCo pseudo-gradients: quant.hip's payload, quantised in
// a randomly rotated basis.  Roofline: HBM (see DESIGN.md §3 "Rotated integer outer step").
//
// Format.  quant.hip's row, byte for byte in layout (ga_quant_row_bytes serves both):
// 256-element blocks, nb = ceil(n / 256),
//   [ q : nb * 256 * bits / 8 ][ scales : nb x fp32 ]      rounded up to 16 bytes
// with q and the scale of a block taken from y = FWHT256(sigma * d) instead of d.  A short
// last block is zero-padded to 256 before the rotation, so all its 256 codes are live.
//
// Sign diagonal.  sigma_i = -1 when bit (i & 31) of fmix32((uint32)(i >> 5) + seed *
// 0x9E3779B9) is set (murmur3's finaliser), else +1; i is the index in the row the kernel
// was handed.  Multiplying by sigma flips the sign bit.
//
// FWHT256(v): 8 stages h = 1, 2, 4, .., 128, in each for every j with bit h clear
//   (v_j, v_{j+h}) <- (v_j + v_{j+h}, v_j - v_{j+h})
// then every value times 2^-4.  Every line is one individually rounded fp32 operation
// (quant_math.h's rn_* helpers; this file is also built without packed fp32 instructions),
// tests/rht_checks.py does the same operations one at a time in numpy.
// Encode, row k, block B (qmax = 127 | 7):
//   d    = master[i] - float(X[k, i]);  d = d + R[k, i] with a residual;  0 past n
//   y    = FWHT256(sigma * d)
//   amax = max over the block of |y|              (on the bit patterns: a NaN wins)
//   !(amax >= 2^-100) or amax not finite:  s = 0, q = 0
//   else  s = amax / qmax, inv = qmax / amax, q = clamp((int)rintf(y * inv), -qmax, qmax)
//   with a residual:  w = FWHT256(float(q) * s);  R[k, i] = d - sigma_i * w_i   for i < n
// Decode + outer step over S payload rows in ascending row order, in the rotated domain:
//   acc = 0; acc = acc + float(q_r) * s_r;   w = FWHT256(acc);   g = (sigma_i * w_i) / divisor
// then quant.hip's outer update (quant_math.h), the new master written to K_out rows.
//
// Both kernels: a wavefront owns a block, lane l holds elements 4l .. 4l + 3.  Stages 1
// and 2 are in-lane; stages 4 .. 128 pair lane l with lane l ^ 1, 2, 4, 8, 16, 32: quad-
// permute DPP (folded into the add), ds_swizzle in bit mode, v_permlane16_swap and
// v_permlane32_swap.  No LDS memory, no atomics.  A lane on the upper side of a stage
// takes partner - own as partner + (-own): the same single rounded operation.
// rht_encode_kernel: quant_encode_kernel's tile walk (a workgroup of 4 waves, 16 blocks,
// all K rows, master loaded once per block).
// diloco_outer_rht_kernel: a workgroup owns 4096 contiguous elements, 4 blocks per wave;
// per block the S rows' payload words (4 | 2 bytes per lane) and one wave-uniform scale
// per row, one transform, then master / momentum and sc1 stores that are each contiguous
// across the wave.
#include "ga_common.h"
#include "quant_math.h"

namespace ga {

constexpr int kRBlock = 256;        // elements per block: one wavefront x 4
constexpr int kRThreads = 256;      // 4 wavefronts
constexpr int kRWaves = kRThreads / 64;
constexpr int kRTileBlocks = 16;    // blocks per workgroup (4096 elements)

typedef unsigned int rht_u2 __attribute__((ext_vector_type(2)));

inline int64_t rht_blocks(int64_t n) { return ceil_div(n, kRBlock); }
inline int64_t rht_row_bytes(int64_t n, int bits) {
    return (rht_blocks(n) * (kRBlock * bits / 8) + 4 * rht_blocks(n) + 15) / 16 * 16;
}

template <int BITS> struct RQMax;
template <> struct RQMax<8> { static constexpr int value = 127; };
template <> struct RQMax<4> { static constexpr int value = 7; };

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// The sign-bit masks of sigma for the lane's elements 4 lane .. 4 lane + 3 of block b:
// the block's 8 sign words are (b * 8 + (lane >> 3)), the lane's bits 4 (lane & 7) + e.
__device__ __forceinline__ void sigma_masks(int64_t b, int lane, uint32_t salt, uint32_t (&sg)[4]) {
    const uint32_t word = fmix32((uint32_t)(b * 8 + (lane >> 3)) + salt) >> (4 * (lane & 7));
#pragma unroll
    for (int e = 0; e < 4; ++e) sg[e] = (word << (31 - e)) & 0x80000000u;
}

// The value lane (l ^ M) holds, M = 1, 2 (quad-permute DPP), 4, 8 (ds_swizzle, bit mode:
// and 0x1f, or 0, xor M).  Every lane of the wave is active wherever this is called.
template <int M> __device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
    if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);  // [1,0,3,2]
    else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);  // [2,3,0,1]
    else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1f | (M << 10));
}

// (the lower lane's value, the upper lane's value) of the pair l, l ^ M for M = 16, 32:
// v_permlane{16,32}_swap of v with itself leaves v[l & ~M] in the first register and
// v[l | M] in the second, in both lanes of the pair.
template <int M> __device__ __forceinline__ rht_u2 lane_pair(uint32_t v) {
    if constexpr (M == 16) return __builtin_amdgcn_permlane16_swap(v, v, false, false);
    else return __builtin_amdgcn_permlane32_swap(v, v, false, false);
}

template <int M> __device__ __forceinline__ uint32_t wave_xor(uint32_t v, int lane) {
    if constexpr (M >= 16) {
        const rht_u2 p = lane_pair<M>(v);
        return (lane & M) ? p.x : p.y;
    } else {
        return lane_xor<M>(v);
    }
}

// One cross-lane stage on the lane's 4 values; neg is 0x80000000 on the upper lane of the
// pair (lane & M) and 0 on the lower: lower = own + partner, upper = partner + (-own).
template <int M> __device__ __forceinline__ void cross_stage(float (&v)[4], uint32_t neg) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t u = __float_as_uint(v[e]);
        if constexpr (M >= 16) {
            const rht_u2 p = lane_pair<M>(u);
            v[e] = rn_add(__uint_as_float(p.x), __uint_as_float(p.y ^ neg));
        } else {
            v[e] = rn_add(__uint_as_float(lane_xor<M>(u)), __uint_as_float(u ^ neg));
        }
    }
}

// FWHT256 over the wave's block.
__device__ __forceinline__ void fwht256(float (&v)[4], int lane) {
    float a = rn_add(v[0], v[1]), b = rn_sub(v[0], v[1]), c = rn_add(v[2], v[3]), d = rn_sub(v[2], v[3]);  // h = 1
    v[0] = rn_add(a, c); v[2] = rn_sub(a, c); v[1] = rn_add(b, d); v[3] = rn_sub(b, d);                   // h = 2
    const uint32_t l = (uint32_t)lane;
    cross_stage<1>(v, (l << 31) & 0x80000000u);
    cross_stage<2>(v, (l << 30) & 0x80000000u);
    cross_stage<4>(v, (l << 29) & 0x80000000u);
    cross_stage<8>(v, (l << 28) & 0x80000000u);
    cross_stage<16>(v, (l << 27) & 0x80000000u);
    cross_stage<32>(v, (l << 26) & 0x80000000u);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = rn_mul(v[e], 0x1p-4f);
}

__device__ __forceinline__ uint32_t wave_umax(uint32_t a, int lane) {
    uint32_t p;
    p = wave_xor<1>(a, lane); a = p > a ? p : a;
    p = wave_xor<2>(a, lane); a = p > a ? p : a;
    p = wave_xor<4>(a, lane); a = p > a ? p : a;
    p = wave_xor<8>(a, lane); a = p > a ? p : a;
    p = wave_xor<16>(a, lane); a = p > a ? p : a;
    p = wave_xor<32>(a, lane); a = p > a ? p : a;
    return a;
}

// X: [K, ld_x] rows of T, master: [n] fp32, R: [K, ld_r] fp32 or null, payload: [K, ld_q] bytes.
// VEC: 16-byte (bf16: 8-byte) loads and stores on whole blocks; the short last block, and
// every block when VEC is false, goes element by element with the same arithmetic.
template <typename T, int BITS, bool VEC>
__global__ __launch_bounds__(kRThreads) void rht_encode_kernel(
    const T* __restrict__ X, int64_t K, int64_t ld_x, const float* __restrict__ master, float* __restrict__ R,
    int64_t ld_r, int64_t n, uint8_t* __restrict__ payload, int64_t ld_q, uint32_t salt) {
    using V = typename Vec4<T>::type;
    constexpr int qmax = RQMax<BITS>::value;
    constexpr int kBlockBytes = kRBlock * BITS / 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nb = (n + kRBlock - 1) / kRBlock;
    const int64_t q_bytes = nb * kBlockBytes;
    const int64_t row_bytes = (q_bytes + 4 * nb + 15) / 16 * 16;
    for (int t = 0; t < kRTileBlocks / kRWaves; ++t) {
        const int64_t b = (int64_t)blockIdx.x * kRTileBlocks + t * kRWaves + wave;  // wave-uniform
        if (b >= nb) break;
        const int64_t i0 = b * kRBlock + 4 * lane;
        const bool whole = VEC && (b + 1) * kRBlock <= n;
        uint32_t sg[4];
        sigma_masks(b, lane, salt, sg);
        float m[4] = {0.f, 0.f, 0.f, 0.f};
        if (whole) {
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(master + i0)), m);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < n) m[e] = master[i0 + e];
        }
        for (int64_t k = 0; k < K; ++k) {
            const T* x = X + k * ld_x;
            float* r = R ? R + k * ld_r : nullptr;
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (whole) {
                float f[4];
                Vec4<T>::unpack(stream_load(reinterpret_cast<const V*>(x + i0)), f);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = rn_sub(m[e], f[e]);
                if (r) {
                    Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(r + i0)), f);
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = rn_add(d[e], f[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (i0 + e < n) {
                        d[e] = rn_sub(m[e], Elem<T>::load(x + i0 + e));
                        if (r) d[e] = rn_add(d[e], r[i0 + e]);
                    }
                }
            }
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = __uint_as_float(__float_as_uint(d[e]) ^ sg[e]);
            fwht256(y, lane);
            // block absmax on the magnitude bits (unsigned order = magnitude order, NaN on top)
            uint32_t a = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t u = __float_as_uint(y[e]) & 0x7FFFFFFFu;
                a = u > a ? u : a;
            }
            a = wave_umax(a, lane);
            float s = 0.f;
            int q[4] = {0, 0, 0, 0};
            if (a >= 0x0D800000u && a < 0x7F800000u) {  // 2^-100 <= amax < inf
                const float amax = __uint_as_float(a);
                s = rn_div(amax, (float)qmax);
                const float inv = rn_div((float)qmax, amax);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int v = (int)rintf(rn_mul(y[e], inv));
                    q[e] = v < -qmax ? -qmax : (v > qmax ? qmax : v);
                }
            }
            uint8_t* row = payload + k * ld_q;
            uint8_t* qb = row + b * kBlockBytes;  // 128 / 256 bytes of this block, 16-byte aligned
            if constexpr (BITS == 8) {
                const uint32_t w = ((uint32_t)q[0] & 0xffu) | (((uint32_t)q[1] & 0xffu) << 8) |
                                   (((uint32_t)q[2] & 0xffu) << 16) | (((uint32_t)q[3] & 0xffu) << 24);
                reinterpret_cast<uint32_t*>(qb)[lane] = w;
            } else {
                const uint32_t h = ((uint32_t)q[0] & 0xfu) | (((uint32_t)q[1] & 0xfu) << 4) |
                                   (((uint32_t)q[2] & 0xfu) << 8) | (((uint32_t)q[3] & 0xfu) << 12);
                const uint32_t up = lane_xor<1>(h);  // the odd neighbour's half
                if (!(lane & 1)) reinterpret_cast<uint32_t*>(qb)[lane >> 1] = h | (up << 16);
            }
            if (lane == 0) reinterpret_cast<float*>(row + q_bytes)[b] = s;
            // the pad behind the scales (0, 4, 8 or 12 bytes), by the wave of the last block
            if (b == nb - 1) {
                const int pad = (int)(row_bytes - q_bytes - 4 * nb) >> 2;
                if (lane >= 1 && lane <= pad) reinterpret_cast<uint32_t*>(row + q_bytes + 4 * nb)[lane - 1] = 0u;
            }
            if (r) {
                float w[4], o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = rn_mul((float)q[e], s);
                fwht256(w, lane);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rn_sub(d[e], __uint_as_float(__float_as_uint(w[e]) ^ sg[e]));
                if (whole) {
                    stream_store(reinterpret_cast<float4*>(r + i0), Vec4<float>::pack(o));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (i0 + e < n) r[i0 + e] = o[e];
                }
            }
        }
    }
}

template <int BITS> __device__ __forceinline__ int rht_sext(uint32_t v) {
    return (int)(v << (32 - BITS)) >> (32 - BITS);
}

// The lane's 4 codes of one block of a payload row: its dword (int8) or half-word (int4).
template <int BITS> __device__ __forceinline__ uint32_t load_codes(const uint8_t* qb, int lane) {
    if constexpr (BITS == 8) return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(qb) + lane);
    else return __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(qb) + lane);
}

// VEC: 16-byte master / momentum access and 16-byte (bf16: 8-byte) sc1 row stores on
// whole blocks; the short last block, and every block when VEC is false, loads and
// stores element by element.  The payload is read by whole blocks either way (rows are
// padded to whole blocks and 16-byte aligned by contract).
template <typename T, int BITS, bool VEC>
__global__ __launch_bounds__(kRThreads) void diloco_outer_rht_kernel(
    const uint8_t* __restrict__ payload, int64_t S, int64_t ld_q, int64_t n, float* master, float* mom,
    QuantOuterParams op, T* dst, int64_t K_out, int64_t ld_dst, uint32_t salt) {
    using V = typename Vec4<T>::type;
    constexpr int kBlockBytes = kRBlock * BITS / 8;
    const bool has_mom = op.momentum != 0.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nb = (n + kRBlock - 1) / kRBlock;
    const int64_t q_bytes = nb * kBlockBytes;
    const int64_t lo = (int64_t)blockIdx.x * kRTileBlocks * kRBlock;  // the workgroup's first element
    for (int t = 0; t < kRTileBlocks / kRWaves; ++t) {
        const int lb = t * kRWaves + wave;  // the block inside the workgroup's span, wave-uniform
        const int64_t b = (int64_t)blockIdx.x * kRTileBlocks + lb;
        if (b >= nb) break;
        const int64_t i0 = b * kRBlock + 4 * lane;
        const bool whole = VEC && (b + 1) * kRBlock <= n;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int64_t r = 0; r < S; ++r) {
            const uint8_t* row = payload + r * ld_q;
            const uint32_t w = load_codes<BITS>(row + b * kBlockBytes, lane);
            const float s = reinterpret_cast<const float*>(row + q_bytes)[b];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                acc[e] = rn_add(acc[e], rn_mul((float)rht_sext<BITS>(w >> (BITS * e)), s));
        }
        fwht256(acc, lane);
        uint32_t sg[4];
        sigma_masks(b, lane, salt, sg);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __uint_as_float(__float_as_uint(acc[e]) ^ sg[e]);
        float m[4] = {0.f, 0.f, 0.f, 0.f}, bf[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
        if (whole) {
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(master + i0)), m);
            if (has_mom && !op.first_step) Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(mom + i0)), bf);
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = quant_outer_update(acc[e], m[e], bf[e], op);
            // device-scope (sc1) stores based at the workgroup's span of each stream
            const uint32_t i = (uint32_t)(lb * 64 + lane);
            store_sc1(reinterpret_cast<float4*>(master + lo), i, Vec4<float>::pack(m));
            if (has_mom) store_sc1(reinterpret_cast<float4*>(mom + lo), i, Vec4<float>::pack(bf));
            const V o = Vec4<T>::pack(out);
            for (int64_t j = 0; j < K_out; ++j) store_sc1(reinterpret_cast<V*>(dst + j * ld_dst + lo), i, o);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (i0 + e < n) {
                    m[e] = master[i0 + e];
                    if (has_mom && !op.first_step) bf[e] = mom[i0 + e];
                    out[e] = quant_outer_update(acc[e], m[e], bf[e], op);
                    master[i0 + e] = m[e];
                    if (has_mom) mom[i0 + e] = bf[e];
                    for (int64_t j = 0; j < K_out; ++j) Elem<T>::store(dst + j * ld_dst + i0 + e, out[e]);
                }
            }
        }
    }
}

static bool r_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

template <typename T, int BITS>
static int launch_rht_encode(const void* x, int64_t K, int64_t ld_x, const float* master, float* residual,
                             int64_t ld_r, int64_t n, uint8_t* payload, int64_t ld_q, uint32_t salt,
                             hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = r_aligned(x, vb) && (K == 1 || ld_x % 4 == 0) && r_aligned(master, 16) &&
                     r_aligned(residual, 16) && (K == 1 || residual == nullptr || ld_r % 4 == 0);
    const dim3 grid((unsigned)ceil_div(rht_blocks(n), kRTileBlocks));
    if (vec)
        hipLaunchKernelGGL((rht_encode_kernel<T, BITS, true>), grid, dim3(kRThreads), 0, stream, (const T*)x, K, ld_x,
                           master, residual, ld_r, n, payload, ld_q, salt);
    else
        hipLaunchKernelGGL((rht_encode_kernel<T, BITS, false>), grid, dim3(kRThreads), 0, stream, (const T*)x, K, ld_x,
                           master, residual, ld_r, n, payload, ld_q, salt);
    return check_launch("ga_rht_encode");
}

template <typename T, int BITS>
static int launch_outer_rht(const uint8_t* payload, int64_t S, int64_t ld_q, int64_t n, float* master, float* mom,
                            const QuantOuterParams& op, void* dst, int64_t K_out, int64_t ld_dst, uint32_t salt,
                            hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = (K_out <= 1 || ld_dst % 4 == 0) && r_aligned(dst, vb) && r_aligned(master, 16) &&
                     r_aligned(mom, 16);
    const dim3 grid((unsigned)ceil_div(rht_blocks(n), kRTileBlocks));
    if (vec)
        hipLaunchKernelGGL((diloco_outer_rht_kernel<T, BITS, true>), grid, dim3(kRThreads), 0, stream, payload, S,
                           ld_q, n, master, mom, op, (T*)dst, K_out, ld_dst, salt);
    else
        hipLaunchKernelGGL((diloco_outer_rht_kernel<T, BITS, false>), grid, dim3(kRThreads), 0, stream, payload, S,
                           ld_q, n, master, mom, op, (T*)dst, K_out, ld_dst, salt);
    return check_launch("ga_diloco_outer_rht");
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int ga_rht_encode(int dtype, const void* x, int64_t K, int64_t ld_x, const float* master,
                                    float* residual, int64_t ld_r, int64_t n, int bits, void* payload,
                                    int64_t ld_q_bytes, uint32_t seed, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_rht_encode: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    GA_REQUIRE(bits == 4 || bits == 8, "ga_rht_encode: bits %d is not 4 or 8", bits);
    if (n == 0) return GA_OK;
    GA_REQUIRE(x && master && payload, "ga_rht_encode: null x/master/payload");
    GA_REQUIRE(K == 1 || ld_x >= n, "ga_rht_encode: ld_x < n");
    GA_REQUIRE(K == 1 || residual == nullptr || ld_r >= n, "ga_rht_encode: ld_r < n");
    GA_REQUIRE(ld_q_bytes >= rht_row_bytes(n, bits) && ld_q_bytes % 16 == 0,
               "ga_rht_encode: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)rht_row_bytes(n, bits));
    GA_REQUIRE(r_aligned(payload, 16), "ga_rht_encode: the payload is not 16-byte aligned");
    GA_REQUIRE(r_aligned(master, 4) && r_aligned(residual, 4), "ga_rht_encode: master/residual not 4-byte aligned");
    uint8_t* pl = (uint8_t*)payload;
    const uint32_t salt = seed * 0x9E3779B9u;
    switch (dtype) {
        case GA_F32:
            return bits == 8 ? launch_rht_encode<float, 8>(x, K, ld_x, master, residual, ld_r, n, pl, ld_q_bytes, salt,
                                                           stream)
                             : launch_rht_encode<float, 4>(x, K, ld_x, master, residual, ld_r, n, pl, ld_q_bytes, salt,
                                                           stream);
        case GA_BF16:
            return bits == 8 ? launch_rht_encode<__hip_bfloat16, 8>(x, K, ld_x, master, residual, ld_r, n, pl,
                                                                    ld_q_bytes, salt, stream)
                             : launch_rht_encode<__hip_bfloat16, 4>(x, K, ld_x, master, residual, ld_r, n, pl,
                                                                    ld_q_bytes, salt, stream);
        default:
            set_error("ga_rht_encode: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_rht(const void* payload, int64_t S, int64_t ld_q_bytes, int bits, int64_t n,
                                          float divisor, float* master, float* mom, int first_step, float lr,
                                          float momentum, float dampening, float weight_decay, int nesterov,
                                          int dtype, void* dst, int64_t K_out, int64_t ld_dst, uint32_t seed,
                                          hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && S >= 1 && K_out >= 0, "ga_diloco_outer_rht: bad sizes n=%lld S=%lld K_out=%lld",
               (long long)n, (long long)S, (long long)K_out);
    GA_REQUIRE(bits == 4 || bits == 8, "ga_diloco_outer_rht: bits %d is not 4 or 8", bits);
    if (n == 0) return GA_OK;
    GA_REQUIRE(payload && master, "ga_diloco_outer_rht: null payload/master");
    GA_REQUIRE(K_out == 0 || dst, "ga_diloco_outer_rht: null dst");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_rht: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(K_out <= 1 || ld_dst >= n, "ga_diloco_outer_rht: ld_dst < n");
    GA_REQUIRE(ld_q_bytes >= rht_row_bytes(n, bits) && ld_q_bytes % 16 == 0,
               "ga_diloco_outer_rht: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)rht_row_bytes(n, bits));
    GA_REQUIRE(r_aligned(payload, 16), "ga_diloco_outer_rht: the payload is not 16-byte aligned");
    GA_REQUIRE(r_aligned(master, 4) && r_aligned(mom, 4), "ga_diloco_outer_rht: master/mom not 4-byte aligned");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_rht: divisor is 0");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_rht: Nesterov momentum requires a momentum and zero dampening");
    QuantOuterParams op{divisor, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    const uint8_t* pl = (const uint8_t*)payload;
    const uint32_t salt = seed * 0x9E3779B9u;
    switch (dtype) {
        case GA_F32:
            return bits == 8 ? launch_outer_rht<float, 8>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out, ld_dst,
                                                          salt, stream)
                             : launch_outer_rht<float, 4>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out, ld_dst,
                                                          salt, stream);
        case GA_BF16:
            return bits == 8 ? launch_outer_rht<__hip_bfloat16, 8>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out,
                                                                   ld_dst, salt, stream)
                             : launch_outer_rht<__hip_bfloat16, 4>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out,
                                                                   ld_dst, salt, stream);
        default:
            set_error("ga_diloco_outer_rht: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}
