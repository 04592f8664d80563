// Block-quantised DiLoCo pseudo-gradients: the int8 / int4 wire (and memory) format
// of the outer step.  Roofline: HBM (see DESIGN.md §3 "Quantised outer step").
//
// Format.  Blocks are 256 consecutive elements of an arena row, nb = ceil(n / 256),
// the last one may be short.  One payload row per node, in bytes:
//   [ q : nb * 256 * bits / 8 ][ scales : nb x fp32 ]      rounded up to 16 bytes
// int8: one two's-complement byte per element; int4: byte j of a block holds element
// 2j in bits 0-3 and element 2j + 1 in bits 4-7 (two's-complement nibbles).  Elements
// past n in the last block and the pad bytes are written as 0.
//
// Arithmetic.  Every line is one individually rounded fp32 operation (rn_add / rn_sub /
// rn_mul / rn_div below, or an explicit fmaf: nothing here may be contracted,
// tests/quant_checks.py does the same operations one at a time in numpy).
// Encode, row k, element i, block b (qmax = 127 | 7):
//   d    = master[i] - float(X[k, i])
//   d    = d + R[k, i]                          with a residual (error feedback)
//   amax = max over the block of |d|
//   !(amax >= 2^-100):  s = 0, q = 0    else    s = amax / qmax, inv = qmax / amax,
//                                               q = clamp((int)rintf(d * inv), -qmax, qmax)
//   R[k, i] = d - float(q) * s                  (mul, then sub)
// Decode + outer step over S payload rows in ascending row order:
//   acc = 0; acc = acc + float(q_r) * s_r;   g = acc / divisor
// then ga_diloco_outer's update of master / momentum on that g (reduce.hip's
// outer_update after its `g = master - avg`), the new master written to K_out rows.
//
// quant_encode_kernel: one wavefront owns one block (a lane's 4 elements are 4l..4l+3),
// the block absmax is a 64-lane butterfly (__shfl_xor: no LDS, no atomics); a workgroup
// walks its tile of 16 blocks for all K rows, so master is loaded once per block.
// diloco_outer_dequant_kernel: the geometry of diloco_outer_kernel (a workgroup owns
// 1024 vectors, sc1 stores), 4 / 2 payload bytes and one block scale per lane and row.
#include "ga_common.h"

namespace ga {

constexpr int kQBlock = 256;        // elements per quantisation block
constexpr int kQThreads = 256;      // 4 wavefronts
constexpr int kQWaves = kQThreads / 64;
constexpr int kQTileBlocks = 16;    // blocks per workgroup tile (4096 elements, reduce.hip's chunk)
constexpr int64_t kQChunk = 1024;   // vectors (or scalars) per workgroup of the decode

inline int64_t quant_blocks(int64_t n) { return ceil_div(n, kQBlock); }
inline int64_t quant_q_bytes(int64_t n, int bits) { return quant_blocks(n) * (kQBlock * bits / 8); }
inline int64_t quant_row_bytes(int64_t n, int bits) {
    return (quant_q_bytes(n, bits) + 4 * quant_blocks(n) + 15) / 16 * 16;
}

template <int BITS> struct QMax;
template <> struct QMax<8> { static constexpr int value = 127; };
template <> struct QMax<4> { static constexpr int value = 7; };

// One correctly rounded fp32 operation that no neighbour can be fused into.  hipcc
// contracts a * b + c across statements by default (-ffp-contract=fast-honor-pragmas),
// and its __fadd_rn / __fmul_rn are the plain operators under that default, so each
// operation is built here with contraction off.
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

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// X: [K, ld_x] rows of T, master: [n] fp32, R: [K, ld_r] fp32 or null, payload: [K, ld_q] bytes.
// VEC: 16-byte (bf16: 8-byte) loads and stores on whole blocks; the short last block, and
// every block when VEC is false, goes element by element with the same arithmetic.
template <typename T, int BITS, bool VEC>
__global__ __launch_bounds__(kQThreads) void quant_encode_kernel(
    const T* __restrict__ X, int64_t K, int64_t ld_x, const float* __restrict__ master, float* __restrict__ R,
    int64_t ld_r, int64_t n, uint8_t* __restrict__ payload, int64_t ld_q) {
    using V = typename Vec4<T>::type;
    constexpr int qmax = QMax<BITS>::value;
    constexpr int kBlockBytes = kQBlock * BITS / 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nb = (n + kQBlock - 1) / kQBlock;
    const int64_t q_bytes = nb * kBlockBytes;
    const int64_t row_bytes = (q_bytes + 4 * nb + 15) / 16 * 16;
    for (int t = 0; t < kQTileBlocks / kQWaves; ++t) {
        const int64_t b = (int64_t)blockIdx.x * kQTileBlocks + t * kQWaves + wave;  // wave-uniform
        if (b >= nb) break;
        const int64_t i0 = b * kQBlock + 4 * lane;
        const bool whole = VEC && (b + 1) * kQBlock <= n;
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
            const float amax = wave_max(fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fmaxf(fabsf(d[2]), fabsf(d[3]))));
            float s = 0.f;
            int q[4] = {0, 0, 0, 0};
            if (amax >= 0x1p-100f) {  // false for NaN too
                s = rn_div(amax, (float)qmax);
                const float inv = rn_div((float)qmax, amax);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int v = (int)rintf(rn_mul(d[e], inv));
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
                const uint32_t up = (uint32_t)__shfl_xor((int)h, 1, 64);  // the odd neighbour's half
                if (!(lane & 1)) reinterpret_cast<uint32_t*>(qb)[lane >> 1] = h | (up << 16);
            }
            if (lane == 0) reinterpret_cast<float*>(row + q_bytes)[b] = s;
            // the pad behind the scales (0, 4, 8 or 12 bytes), by the wave of the last block
            if (b == nb - 1) {
                const int pad = (int)(row_bytes - q_bytes - 4 * nb) >> 2;
                if (lane >= 1 && lane <= pad) reinterpret_cast<uint32_t*>(row + q_bytes + 4 * nb)[lane - 1] = 0u;
            }
            if (r) {
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rn_sub(d[e], rn_mul((float)q[e], s));
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

// ga_diloco_outer's element update from the pseudo-gradient on (reduce.hip, outer_update
// after `g = master - avg`); kept apart from that file so its machine code stays as measured.
struct QuantOuterParams {
    float divisor, lr, momentum, dampening, weight_decay;
    int first_step, nesterov;
};

__device__ __forceinline__ float quant_outer_update(float acc, float& master, float& buf,
                                                    const QuantOuterParams& op) {
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

template <int BITS> __device__ __forceinline__ int sext(uint32_t v) {
    return (int)(v << (32 - BITS)) >> (32 - BITS);
}

// The 4 quantised values of vector v (elements 4v..4v+3) of one payload row.
template <int BITS>
__device__ __forceinline__ void load_q4(const uint8_t* row, int64_t v, int (&q)[4]) {
    if constexpr (BITS == 8) {
        const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(row) + v);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = sext<8>(w >> (8 * e));
    } else {
        const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(row) + v);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = sext<4>(w >> (4 * e));
    }
}

template <int BITS>
__device__ __forceinline__ int load_q1(const uint8_t* row, int64_t i) {
    if constexpr (BITS == 8) return sext<8>(row[i]);
    else return sext<4>((uint32_t)row[i >> 1] >> ((i & 1) * 4));
}

template <typename T, int BITS, bool VEC>
__global__ __launch_bounds__(kQThreads) void diloco_outer_dequant_kernel(
    const uint8_t* __restrict__ payload, int64_t S, int64_t ld_q, int64_t n, float* master, float* mom,
    QuantOuterParams op, T* dst, int64_t K_out, int64_t ld_dst) {
    const bool has_mom = op.momentum != 0.f;
    const int64_t q_bytes = (n + kQBlock - 1) / kQBlock * (kQBlock * BITS / 8);
    int64_t lo, hi;
    if constexpr (VEC) {
        using V = typename Vec4<T>::type;
        const int64_t total = n >> 2;
        lo = (int64_t)blockIdx.x * kQChunk;
        hi = lo + kQChunk < total ? lo + kQChunk : total;
        for (int64_t v = lo + threadIdx.x; v < hi; v += kQThreads) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int64_t r = 0; r < S; ++r) {
                const uint8_t* row = payload + r * ld_q;
                int q[4];
                load_q4<BITS>(row, v, q);
                const float s = reinterpret_cast<const float*>(row + q_bytes)[v >> 6];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = rn_add(acc[e], rn_mul((float)q[e], s));
            }
            float m[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(master) + v), m);
            if (has_mom && !op.first_step) Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(mom) + v), b);
            float out[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = quant_outer_update(acc[e], m[e], b[e], op);
            const V o = Vec4<T>::pack(out);
            // device-scope (sc1) stores based at the workgroup's block of each stream
            const uint32_t i = (uint32_t)(v - lo);
            store_sc1(reinterpret_cast<float4*>(master) + lo, i, Vec4<float>::pack(m));
            if (has_mom) store_sc1(reinterpret_cast<float4*>(mom) + lo, i, Vec4<float>::pack(b));
            for (int64_t j = 0; j < K_out; ++j) store_sc1(reinterpret_cast<V*>(dst + j * ld_dst) + lo, i, o);
        }
    } else {
        lo = (int64_t)blockIdx.x * kQChunk;
        hi = lo + kQChunk < n ? lo + kQChunk : n;
        for (int64_t i = lo + threadIdx.x; i < hi; i += kQThreads) {
            float acc = 0.f;
#pragma unroll 4
            for (int64_t r = 0; r < S; ++r) {
                const uint8_t* row = payload + r * ld_q;
                const float s = reinterpret_cast<const float*>(row + q_bytes)[i >> 8];
                acc = rn_add(acc, rn_mul((float)load_q1<BITS>(row, i), s));
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

static bool q_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

template <typename T, int BITS>
static int launch_quant_encode(const void* x, int64_t K, int64_t ld_x, const float* master, float* residual,
                               int64_t ld_r, int64_t n, uint8_t* payload, int64_t ld_q, hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = q_aligned(x, vb) && (K == 1 || ld_x % 4 == 0) && q_aligned(master, 16) &&
                     q_aligned(residual, 16) && (K == 1 || residual == nullptr || ld_r % 4 == 0);
    const dim3 grid((unsigned)ceil_div(quant_blocks(n), kQTileBlocks));
    if (vec)
        hipLaunchKernelGGL((quant_encode_kernel<T, BITS, true>), grid, dim3(kQThreads), 0, stream, (const T*)x, K,
                           ld_x, master, residual, ld_r, n, payload, ld_q);
    else
        hipLaunchKernelGGL((quant_encode_kernel<T, BITS, false>), grid, dim3(kQThreads), 0, stream, (const T*)x, K,
                           ld_x, master, residual, ld_r, n, payload, ld_q);
    return check_launch("ga_quant_encode");
}

template <typename T, int BITS>
static int launch_outer_dequant(const uint8_t* payload, int64_t S, int64_t ld_q, int64_t n, float* master,
                                float* mom, const QuantOuterParams& op, void* dst, int64_t K_out, int64_t ld_dst,
                                hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = (n % 4 == 0) && (K_out <= 1 || ld_dst % 4 == 0) && q_aligned(dst, vb) &&
                     q_aligned(master, 16) && q_aligned(mom, 16);
    if (vec)
        hipLaunchKernelGGL((diloco_outer_dequant_kernel<T, BITS, true>), dim3((unsigned)ceil_div(n / 4, kQChunk)),
                           dim3(kQThreads), 0, stream, payload, S, ld_q, n, master, mom, op, (T*)dst, K_out, ld_dst);
    else
        hipLaunchKernelGGL((diloco_outer_dequant_kernel<T, BITS, false>), dim3((unsigned)ceil_div(n, kQChunk)),
                           dim3(kQThreads), 0, stream, payload, S, ld_q, n, master, mom, op, (T*)dst, K_out, ld_dst);
    return check_launch("ga_diloco_outer_dequant");
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int64_t ga_quant_row_bytes(int64_t n, int bits) {
    if (n < 0 || (bits != 4 && bits != 8)) return -1;
    return quant_row_bytes(n, bits);
}

extern "C" GA_API int ga_quant_encode(int dtype, const void* x, int64_t K, int64_t ld_x, const float* master,
                                      float* residual, int64_t ld_r, int64_t n, int bits, void* payload,
                                      int64_t ld_q_bytes, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && K >= 1, "ga_quant_encode: bad sizes n=%lld K=%lld", (long long)n, (long long)K);
    GA_REQUIRE(bits == 4 || bits == 8, "ga_quant_encode: bits %d is not 4 or 8", bits);
    if (n == 0) return GA_OK;
    GA_REQUIRE(x && master && payload, "ga_quant_encode: null x/master/payload");
    GA_REQUIRE(K == 1 || ld_x >= n, "ga_quant_encode: ld_x < n");
    GA_REQUIRE(K == 1 || residual == nullptr || ld_r >= n, "ga_quant_encode: ld_r < n");
    GA_REQUIRE(ld_q_bytes >= quant_row_bytes(n, bits) && ld_q_bytes % 16 == 0,
               "ga_quant_encode: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)quant_row_bytes(n, bits));
    GA_REQUIRE(q_aligned(payload, 16), "ga_quant_encode: the payload is not 16-byte aligned");
    GA_REQUIRE(q_aligned(master, 4) && q_aligned(residual, 4), "ga_quant_encode: master/residual not 4-byte aligned");
    uint8_t* pl = (uint8_t*)payload;
    switch (dtype) {
        case GA_F32:
            return bits == 8 ? launch_quant_encode<float, 8>(x, K, ld_x, master, residual, ld_r, n, pl, ld_q_bytes,
                                                             stream)
                             : launch_quant_encode<float, 4>(x, K, ld_x, master, residual, ld_r, n, pl, ld_q_bytes,
                                                             stream);
        case GA_BF16:
            return bits == 8 ? launch_quant_encode<__hip_bfloat16, 8>(x, K, ld_x, master, residual, ld_r, n, pl,
                                                                      ld_q_bytes, stream)
                             : launch_quant_encode<__hip_bfloat16, 4>(x, K, ld_x, master, residual, ld_r, n, pl,
                                                                      ld_q_bytes, stream);
        default:
            set_error("ga_quant_encode: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}

extern "C" GA_API int ga_diloco_outer_dequant(const void* payload, int64_t S, int64_t ld_q_bytes, int bits,
                                              int64_t n, float divisor, float* master, float* mom, int first_step,
                                              float lr, float momentum, float dampening, float weight_decay,
                                              int nesterov, int dtype, void* dst, int64_t K_out, int64_t ld_dst,
                                              hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && S >= 1 && K_out >= 0, "ga_diloco_outer_dequant: bad sizes n=%lld S=%lld K_out=%lld",
               (long long)n, (long long)S, (long long)K_out);
    GA_REQUIRE(bits == 4 || bits == 8, "ga_diloco_outer_dequant: bits %d is not 4 or 8", bits);
    if (n == 0) return GA_OK;
    GA_REQUIRE(payload && master, "ga_diloco_outer_dequant: null payload/master");
    GA_REQUIRE(K_out == 0 || dst, "ga_diloco_outer_dequant: null dst");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_dequant: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(K_out <= 1 || ld_dst >= n, "ga_diloco_outer_dequant: ld_dst < n");
    GA_REQUIRE(ld_q_bytes >= quant_row_bytes(n, bits) && ld_q_bytes % 16 == 0,
               "ga_diloco_outer_dequant: ld_q_bytes %lld is less than the row's %lld bytes or not a multiple of 16",
               (long long)ld_q_bytes, (long long)quant_row_bytes(n, bits));
    GA_REQUIRE(q_aligned(payload, 16), "ga_diloco_outer_dequant: the payload is not 16-byte aligned");
    GA_REQUIRE(q_aligned(master, 4) && q_aligned(mom, 4), "ga_diloco_outer_dequant: master/mom not 4-byte aligned");
    GA_REQUIRE(divisor != 0.0f, "ga_diloco_outer_dequant: divisor is 0");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_dequant: Nesterov momentum requires a momentum and zero dampening");
    QuantOuterParams op{divisor, lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    const uint8_t* pl = (const uint8_t*)payload;
    switch (dtype) {
        case GA_F32:
            return bits == 8 ? launch_outer_dequant<float, 8>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out,
                                                              ld_dst, stream)
                             : launch_outer_dequant<float, 4>(pl, S, ld_q_bytes, n, master, mom, op, dst, K_out,
                                                              ld_dst, stream);
        case GA_BF16:
            return bits == 8 ? launch_outer_dequant<__hip_bfloat16, 8>(pl, S, ld_q_bytes, n, master, mom, op, dst,
                                                                       K_out, ld_dst, stream)
                             : launch_outer_dequant<__hip_bfloat16, 4>(pl, S, ld_q_bytes, n, master, mom, op, dst,
                                                                       K_out, ld_dst, stream);
        default:
            set_error("ga_diloco_outer_dequant: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}
