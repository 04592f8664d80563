// MX block-float DiLoCo pseudo-gradients: the mxfp8 (E4M3) / mxfp4 (E2M1) wire (and
// memory) format of the outer step.  Roofline: HBM (see DESIGN.md §3 "MX outer step").
//
// Format (OCP MX, scale rounded up so nothing saturates).  Blocks are 32 consecutive
// elements of an arena row, nb = ceil(n / 32), the last one may be short.  One payload
// row per node, in bytes:
//   [ elements : nb * 32 * bits / 8 ][ scales : nb x E8M0 byte ]   rounded up to 16 bytes
// mxfp8: one E4M3 byte per element (torch's float8_e4m3fn; 0x7F / 0xFF never produced);
// mxfp4: byte j of a block holds element 2j in bits 0-3 and element 2j + 1 in bits 4-7
// (E2M1, bit 3 of the nibble the sign).  A scale byte b stands for 2^(b - 127).  Elements
// past n in the last block and the pad bytes are written as 0.
//
// Arithmetic.  Every line is one individually rounded fp32 operation (quant_math.h's
// rn_* helpers; this file is also built without packed fp32 instructions),
// tests/mx_checks.py does the same operations one at a time in numpy.
// Encode, row k, element i, block B (emax = 8 | 2, the exponent of 448 | 6):
//   d    = master[i] - float(X[k, i])
//   d    = d + R[k, i]                          with a residual (error feedback)
//   amax = max over the block of |d|            (on the bit patterns: a NaN wins)
//   !(amax >= 2^-100) or amax not finite:  b = 0, every element +0
//   else  E, M = exponent and mantissa fields of amax
//         b = E - emax + (M > mantissa of 448 | 6)           in 19..253
//         element = d * 2^-(b - 127) rounded to nearest even on the element grid, sign kept
//   R[k, i] = d - element * 2^(b - 127)         (the product is exact)
// Decode + outer step over S payload rows in ascending row order:
//   acc = 0; acc = acc + element_r * 2^(b_r - 127);   g = acc / divisor
// then quant.hip's outer update (quant_math.h), the new master written to K_out rows.
//
// mx_encode_kernel: a lane owns 8 consecutive elements and a quad of 4 lanes one block,
// so the block absmax is two quad-local exchanges (xor 1, xor 2) on the integer
// magnitude bits; the scale byte is integer arithmetic on those bits; the 8 elements go
// through four v_cvt_scalef32_pk_{fp8,fp4}_f32 (8 bytes | one dword per lane, no
// neighbour exchange); a wave covers 512 elements and its 16 scale bytes leave as one
// 16-byte store from lane 0 (two shifts down the wave, then four readlanes).  A workgroup
// walks a 4096-element tile for all K rows, so master is loaded once per tile.  The
// residual comes from the bytes just produced through v_cvt_scalef32_pk_f32_{fp8,fp4}.
// diloco_outer_mx_kernel: the geometry of diloco_outer_kernel (a workgroup owns a
// contiguous span of 4096 elements, sc1 stores), 8 elements per lane: 8 | 4 payload bytes
// and one scale byte per lane and row.
#include "ga_common.h"
#include "quant_math.h"

namespace ga {

constexpr int kMxBlock = 32;          // elements per block
constexpr int kMxThreads = 256;       // 4 wavefronts
constexpr int kMxLaneElems = 8;       // a lane's consecutive elements: a quad owns a block
constexpr int kMxWaveElems = 64 * kMxLaneElems;       // 512: 16 blocks
constexpr int kMxTileWaves = 8;       // wave spans per workgroup tile (4096 elements)
constexpr int64_t kMxChunk = 512;     // lane items (8 elements each) per workgroup of the decode

typedef short mx_s2 __attribute__((ext_vector_type(2)));
typedef float mx_f2 __attribute__((__vector_size__(2 * sizeof(float))));
typedef unsigned int mx_u4 __attribute__((ext_vector_type(4)));

inline int64_t mx_blocks(int64_t n) { return ceil_div(n, kMxBlock); }
inline int64_t mx_e_bytes(int64_t n, int bits) { return mx_blocks(n) * (kMxBlock * bits / 8); }
inline int64_t mx_row_bytes(int64_t n, int bits) { return (mx_e_bytes(n, bits) + mx_blocks(n) + 15) / 16 * 16; }

// The exponent of the largest element (448 = 1.75 * 2^8, 6 = 1.5 * 2^2) and the mantissa
// field above which amax / 2^(E - emax) would pass it.
template <int BITS> struct MxFmt;
template <> struct MxFmt<8> { static constexpr uint32_t emax = 8, mant = 0x600000u; };
template <> struct MxFmt<4> { static constexpr uint32_t emax = 2, mant = 0x400000u; };

// The E8M0 scale byte of a block from the bits of its absmax (sign bit clear); 0 for a
// block below 2^-100 (0x0D800000) or holding an Inf or a NaN.
template <int BITS> __device__ __forceinline__ uint32_t mx_scale_byte(uint32_t amax_bits) {
    if (amax_bits < 0x0D800000u || amax_bits >= 0x7F800000u) return 0u;
    return (amax_bits >> 23) - MxFmt<BITS>::emax + ((amax_bits & 0x7FFFFFu) > MxFmt<BITS>::mant ? 1u : 0u);
}

// The hardware's scale operand of byte b: the fp32 number 2^(b - 127).
__device__ __forceinline__ float mx_scale(uint32_t b) { return __uint_as_float(b << 23); }

// Eight values over 2^(b - 127) to eight element codes: 2 dwords (mxfp8) or 1 (mxfp4).
template <int BITS> struct MxCodes;
template <> struct MxCodes<8> {
    uint32_t w[2];
    __device__ __forceinline__ void encode(const float (&d)[8], float scale) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            mx_s2 v = {0, 0};
            v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, d[4 * h], d[4 * h + 1], scale, false);
            v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, d[4 * h + 2], d[4 * h + 3], scale, true);
            w[h] = (uint32_t)(uint16_t)v.x | ((uint32_t)(uint16_t)v.y << 16);
        }
    }
    __device__ __forceinline__ void decode(float (&f)[8], float scale) const {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const mx_f2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[h], scale, false);
            const mx_f2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[h], scale, true);
            f[4 * h] = lo[0]; f[4 * h + 1] = lo[1]; f[4 * h + 2] = hi[0]; f[4 * h + 3] = hi[1];
        }
    }
    __device__ __forceinline__ void clear() { w[0] = w[1] = 0u; }
    __device__ __forceinline__ void load(const uint8_t* row, int64_t o) {
        const ga_u2 v = __builtin_nontemporal_load(reinterpret_cast<const ga_u2*>(row) + o);
        w[0] = v.x; w[1] = v.y;
    }
    __device__ __forceinline__ void store(uint8_t* row, int64_t o) const {
        ga_u2 v;
        v.x = w[0]; v.y = w[1];
        reinterpret_cast<ga_u2*>(row)[o] = v;
    }
};
template <> struct MxCodes<4> {
    uint32_t w[1];
    __device__ __forceinline__ void encode(const float (&d)[8], float scale) {
        uint32_t v = 0u;
        v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[0], d[1], scale, 0);
        v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[2], d[3], scale, 1);
        v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[4], d[5], scale, 2);
        v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[6], d[7], scale, 3);
        w[0] = v;
    }
    __device__ __forceinline__ void decode(float (&f)[8], float scale) const {
        const mx_f2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 0);
        const mx_f2 b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 1);
        const mx_f2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 2);
        const mx_f2 e = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], scale, 3);
        f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1]; f[4] = c[0]; f[5] = c[1]; f[6] = e[0]; f[7] = e[1];
    }
    __device__ __forceinline__ void clear() { w[0] = 0u; }
    __device__ __forceinline__ void load(const uint8_t* row, int64_t o) {
        w[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(row) + o);
    }
    __device__ __forceinline__ void store(uint8_t* row, int64_t o) const { reinterpret_cast<uint32_t*>(row)[o] = w[0]; }
};

// One element's code of a payload row (the decode's element path), in the low bits.
template <int BITS> __device__ __forceinline__ float mx_load_one(const uint8_t* row, int64_t i, float scale) {
    if constexpr (BITS == 8) {
        return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((uint32_t)row[i], scale, false)[0];
    } else {
        const uint32_t nib = ((uint32_t)row[i >> 1] >> ((i & 1) * 4)) & 0xfu;
        return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(nib, scale, 0)[0];
    }
}

// 8 consecutive elements of a row: two 16-byte loads (fp32) or one (bf16).
__device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
    const float4 a = stream_load(reinterpret_cast<const float4*>(p));
    const float4 b = stream_load(reinterpret_cast<const float4*>(p) + 1);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ void load8(const __hip_bfloat16* p, float (&f)[8]) {
    const mx_u4 v = __builtin_nontemporal_load(reinterpret_cast<const mx_u4*>(p));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = __uint_as_float(w[e] << 16);
        f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
    }
}

// X: [K, ld_x] rows of T, master: [n] fp32, R: [K, ld_r] fp32 or null, payload: [K, ld_q] bytes.
// VEC: 16-byte loads and stores on whole blocks; the short last block, and every block
// when VEC is false, reads and writes x / master / R element by element with the same
// arithmetic.  The payload is 16-byte aligned and padded to whole blocks either way.
template <typename T, int BITS, bool VEC>
__global__ __launch_bounds__(kMxThreads) void mx_encode_kernel(
    const T* __restrict__ X, int64_t K, int64_t ld_x, const float* __restrict__ master, float* __restrict__ R,
    int64_t ld_r, int64_t n, uint8_t* __restrict__ payload, int64_t ld_q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nb = (n + kMxBlock - 1) / kMxBlock;
    const int64_t e_bytes = nb * (kMxBlock * BITS / 8);
    for (int t = 0; t < kMxTileWaves / (kMxThreads / 64); ++t) {
        const int64_t w = (int64_t)blockIdx.x * kMxTileWaves + t * (kMxThreads / 64) + wave;  // wave-uniform
        if (w * kMxWaveElems >= n) break;
        const int64_t o = w * 64 + lane;           // the lane's item: elements 8o .. 8o + 7
        const int64_t i0 = o * kMxLaneElems;
        const int64_t blk = o >> 2;                // quad-uniform
        const bool whole = VEC && (blk + 1) * kMxBlock <= n;
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (whole) {
            load8(master + i0, m);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (i0 + e < n) m[e] = master[i0 + e];
        }
        for (int64_t k = 0; k < K; ++k) {
            const T* x = X + k * ld_x;
            float* r = R ? R + k * ld_r : nullptr;
            float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (whole) {
                float f[8];
                load8(x + i0, f);
#pragma unroll
                for (int e = 0; e < 8; ++e) d[e] = rn_sub(m[e], f[e]);
                if (r) {
                    load8(r + i0, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) d[e] = rn_add(d[e], f[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (i0 + e < n) {
                        d[e] = rn_sub(m[e], Elem<T>::load(x + i0 + e));
                        if (r) d[e] = rn_add(d[e], r[i0 + e]);
                    }
                }
            }
            // block absmax on the magnitude bits (unsigned order = magnitude order, NaN on top)
            uint32_t a = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t u = __float_as_uint(d[e]) & 0x7FFFFFFFu;
                a = u > a ? u : a;
            }
            uint32_t p = (uint32_t)__shfl_xor((int)a, 1, 64);
            a = p > a ? p : a;
            p = (uint32_t)__shfl_xor((int)a, 2, 64);
            a = p > a ? p : a;
            const uint32_t sb = mx_scale_byte<BITS>(a);  // 0 for blocks past nb too (d = 0)
            const float scale = mx_scale(sb);
            MxCodes<BITS> c;
            c.encode(d, scale);
            if (sb == 0u) c.clear();
            uint8_t* row = payload + k * ld_q;
            if (blk < nb) c.store(row, o);
            // the wave's 16 scale bytes (zero past nb: the row's pad) as one 16-byte store
            uint32_t s = sb;
            s |= (uint32_t)__shfl_down((int)s, 4, 64) << 8;    // lanes 8j: blocks 2j, 2j + 1
            s |= (uint32_t)__shfl_down((int)s, 8, 64) << 16;   // lanes 16j: blocks 4j .. 4j + 3
            mx_u4 sv;
            sv.x = (uint32_t)__builtin_amdgcn_readlane((int)s, 0);
            sv.y = (uint32_t)__builtin_amdgcn_readlane((int)s, 16);
            sv.z = (uint32_t)__builtin_amdgcn_readlane((int)s, 32);
            sv.w = (uint32_t)__builtin_amdgcn_readlane((int)s, 48);
            if (lane == 0) *reinterpret_cast<mx_u4*>(row + e_bytes + w * 16) = sv;
            if (r) {
                float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (sb != 0u) c.decode(q, scale);
                float out[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) out[e] = rn_sub(d[e], q[e]);
                if (whole) {
                    stream_store(reinterpret_cast<float4*>(r + i0), make_float4(out[0], out[1], out[2], out[3]));
                    stream_store(reinterpret_cast<float4*>(r + i0) + 1, make_float4(out[4], out[5], out[6], out[7]));
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (i0 + e < n) r[i0 + e] = out[e];
                }
            }
        }
    }
}

// 8 outputs of lane item i of the workgroup's span based at `lo` items: sc1 stores.
__device__ __forceinline__ void store8_sc1(float* base, int64_t lo, uint32_t i, const float (&f)[8]) {
    float4* wg = reinterpret_cast<float4*>(base) + 2 * lo;
    store_sc1(wg, 2 * i, make_float4(f[0], f[1], f[2], f[3]));
    store_sc1(wg, 2 * i + 1, make_float4(f[4], f[5], f[6], f[7]));
}
__device__ __forceinline__ void store8_sc1(__hip_bfloat16* base, int64_t lo, uint32_t i, const float (&f)[8]) {
    uint2* wg = reinterpret_cast<uint2*>(base) + 2 * lo;
    const float a[4] = {f[0], f[1], f[2], f[3]}, b[4] = {f[4], f[5], f[6], f[7]};
    store_sc1(wg, 2 * i, Vec4<__hip_bfloat16>::pack(a));
    store_sc1(wg, 2 * i + 1, Vec4<__hip_bfloat16>::pack(b));
}

template <typename T, int BITS, bool VEC>
__global__ __launch_bounds__(kMxThreads) void diloco_outer_mx_kernel(
    const uint8_t* __restrict__ payload, int64_t S, int64_t ld_q, int64_t n, float* master, float* mom,
    QuantOuterParams op, T* dst, int64_t K_out, int64_t ld_dst) {
    const bool has_mom = op.momentum != 0.f;
    const int64_t e_bytes = (n + kMxBlock - 1) / kMxBlock * (kMxBlock * BITS / 8);
    if constexpr (VEC) {
        const int64_t total = n >> 3;
        const int64_t lo = (int64_t)blockIdx.x * kMxChunk;
        const int64_t hi = lo + kMxChunk < total ? lo + kMxChunk : total;
        for (int64_t o = lo + threadIdx.x; o < hi; o += kMxThreads) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int64_t r = 0; r < S; ++r) {
                const uint8_t* row = payload + r * ld_q;
                MxCodes<BITS> c;
                c.load(row, o);
                const uint32_t sb = row[e_bytes + (o >> 2)];
                float q[8];
                c.decode(q, mx_scale(sb));
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = rn_add(acc[e], sb != 0u ? q[e] : 0.f);
            }
            float m[8], b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            load8(master + 8 * o, m);
            if (has_mom && !op.first_step) load8(mom + 8 * o, b);
            float out[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) out[e] = quant_outer_update(acc[e], m[e], b[e], op);
            // device-scope (sc1) stores based at the workgroup's block of each stream
            const uint32_t i = (uint32_t)(o - lo);
            store8_sc1(master, lo, i, m);
            if (has_mom) store8_sc1(mom, lo, i, b);
            for (int64_t j = 0; j < K_out; ++j) store8_sc1(dst + j * ld_dst, lo, i, out);
        }
    } else {
        const int64_t lo = (int64_t)blockIdx.x * kMxChunk * kMxLaneElems;
        const int64_t span = kMxChunk * kMxLaneElems;
        const int64_t hi = lo + span < n ? lo + span : n;
        for (int64_t i = lo + threadIdx.x; i < hi; i += kMxThreads) {
            float acc = 0.f;
#pragma unroll 4
            for (int64_t r = 0; r < S; ++r) {
                const uint8_t* row = payload + r * ld_q;
                const uint32_t sb = row[e_bytes + (i >> 5)];
                const float q = mx_load_one<BITS>(row, i, mx_scale(sb));
                acc = rn_add(acc, sb != 0u ? q : 0.f);
            }
            float m = master[i];
            float b = (has_mom && !op.first_step) ? mom[i] : 0.f;
            const float out = quant_outer_update(acc, m, b, op);
            master[i] = m;
            if (has_mom) mom[i] = b;
            for (int64_t j = 0; j < K_out; ++j) Elem<T>::store(dst + j * ld_dst + i, out);
        }
    }
}

static bool mx_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

template <typename T, int BITS>
static int launch_mx_encode(const void* x, int64_t K, int64_t ld_x, const float* master, float* residual,
                            int64_t ld_r, int64_t n, uint8_t* payload, int64_t ld_q, hipStream_t stream) {
    // a lane's 8 elements are 16-byte loads at 8 * sizeof(T)-byte offsets: 16-byte bases, ld % (16 / sizeof(T))
    const int ldm = 16 / (int)sizeof(T);
    const bool vec = mx_aligned(x, 16) && (K == 1 || ld_x % ldm == 0) && mx_aligned(master, 16) &&
                     mx_aligned(residual, 16) && (K == 1 || residual == nullptr || ld_r % 4 == 0);
    const dim3 grid((unsigned)ceil_div(n, (int64_t)kMxTileWaves * kMxWaveElems));
    if (vec)
        hipLaunchKernelGGL((mx_encode_kernel<T, BITS, true>), grid, dim3(kMxThreads), 0, stream, (const T*)x, K, ld_x,
                           master, residual, ld_r, n, payload, ld_q);
    else
        hipLaunchKernelGGL((mx_encode_kernel<T, BITS, false>), grid, dim3(kMxThreads), 0, stream, (const T*)x, K, ld_x,
                           master, residual, ld_r, n, payload, ld_q);
    return check_launch("ga_mx_encode");
}

template <typename T, int BITS>
static int launch_outer_mx(const uint8_t* payload, int64_t S, int64_t ld_q, int64_t n, float* master, float* mom,
                           const QuantOuterParams& op, void* dst, int64_t K_out, int64_t ld_dst, hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);  // the dst rows go out as 4-element vectors
    const bool vec = (n % 8 == 0) && (K_out <= 1 || ld_dst % 4 == 0) && mx_aligned(dst, vb) &&
                     mx_aligned(master, 16) && mx_aligned(mom, 16);
    const dim3 grid((unsigned)ceil_div(n, kMxChunk * kMxLaneElems));
    if (vec)
        hipLaunchKernelGGL((diloco_outer_mx_kernel<T, BITS, true>), grid, dim3(kMxThreads), 0, stream, payload, S,
                           ld_q, n, master, mom, op, (T*)dst, K_out, ld_dst);
    else
        hipLaunchKernelGGL((diloco_outer_mx_kernel<T, BITS, false>), grid, dim3(kMxThreads), 0, stream, payload, S,
                           ld_q, n, master, mom, op, (T*)dst, K_out, ld_dst);
    return check_launch("ga_diloco_outer_mx");
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int64_t ga_mx_row_bytes(int64_t n, int bits) {
    if (n < 0 || (bits != 4 && bits != 8)) return -1;
    return mx_row_bytes(n, bits);
}

extern "C" GA_API int ga_mx_encode(int dtype, const void* x, int64_t K, int64_t ld_x, const float* master,
                                   float* residual, int64_t ld_r, int64_t n, int bits, void* payload,
                                   int64_t ld_q_bytes, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_mx_encode: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    GA_REQUIRE(bits == 4 || bits == 8, "ga_mx_encode: bits %d is not 4 or 8", bits);
    if (n == 0) return GA_OK;
    GA_REQUIRE(x && master && payload, "ga_mx_encode: null x/master/payload");
    GA_REQUIRE(K == 1 || ld_x >= n, "ga_mx_encode: ld_x < n");
    GA_REQUIRE(K == 1 || residual == nullptr || ld_r >= n, "ga_mx_encode: ld_r < n");
    GA_REQUIRE(ld_q_bytes >= mx_row_bytes(n, bits) && ld_q_bytes % 16 == 0,
               "ga_mx_encode: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)mx_row_bytes(n, bits));
    GA_REQUIRE(mx_aligned(payload, 16), "ga_mx_encode: the payload is not 16-byte aligned");
    GA_REQUIRE(mx_aligned(master, 4) && mx_aligned(residual, 4), "ga_mx_encode: master/residual not 4-byte aligned");
    uint8_t* pl = (uint8_t*)payload;
    switch (dtype) {
        case GA_F32:
            return bits == 8 ? launch_mx_encode<float, 8>(x, K, ld_x, master, residual, ld_r, n, pl, ld_q_bytes, stream)
                             : launch_mx_encode<float, 4>(x, K, ld_x, master, residual, ld_r, n, pl, ld_q_bytes, stream);
        case GA_BF16:
            return bits == 8 ? launch_mx_encode<__hip_bfloat16, 8>(x, K, ld_x, master, residual, ld_r, n, pl,
                                                                   ld_q_bytes, stream)
                             : launch_mx_encode<__hip_bfloat16, 4>(x, K, ld_x, master, residual, ld_r, n, pl,
                                                                   ld_q_bytes, stream);
        default:
            set_error("ga_mx_encode: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_mx(const void* payload, int64_t S, int64_t ld_q_bytes, int bits, int64_t n,
                                         float divisor, float* master, float* mom, int first_step, float lr,
                                         float momentum, float dampening, float weight_decay, int nesterov, int dtype,
                                         void* dst, int64_t K_out, int64_t ld_dst, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && S >= 1 && K_out >= 0, "ga_diloco_outer_mx: bad sizes n=%lld S=%lld K_out=%lld", (long long)n,
               (long long)S, (long long)K_out);
    GA_REQUIRE(bits == 4 || bits == 8, "ga_diloco_outer_mx: bits %d is not 4 or 8", bits);
    if (n == 0) return GA_OK;
    GA_REQUIRE(payload && master, "ga_diloco_outer_mx: null payload/master");
    GA_REQUIRE(K_out == 0 || dst, "ga_diloco_outer_mx: null dst");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_mx: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(K_out <= 1 || ld_dst >= n, "ga_diloco_outer_mx: ld_dst < n");
    GA_REQUIRE(ld_q_bytes >= mx_row_bytes(n, bits) && ld_q_bytes % 16 == 0,
               "ga_diloco_outer_mx: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)mx_row_bytes(n, bits));
    GA_REQUIRE(mx_aligned(payload, 16), "ga_diloco_outer_mx: the payload is not 16-byte aligned");
    GA_REQUIRE(mx_aligned(master, 4) && mx_aligned(mom, 4), "ga_diloco_outer_mx: master/mom not 4-byte aligned");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_mx: divisor is 0");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_mx: Nesterov momentum requires a momentum and zero dampening");
    QuantOuterParams op{divisor, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    const uint8_t* pl = (const uint8_t*)payload;
    switch (dtype) {
        case GA_F32:
            return bits == 8
                       ? launch_outer_mx<float, 8>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out, ld_dst, stream)
                       : launch_outer_mx<float, 4>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out, ld_dst, stream);
        case GA_BF16:
            return bits == 8 ? launch_outer_mx<__hip_bfloat16, 8>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out,
                                                                  ld_dst, stream)
                             : launch_outer_mx<__hip_bfloat16, 4>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out,
                                                                  ld_dst, stream);
        default:
            set_error("ga_diloco_outer_mx: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}
