// The island outer step (ga_diloco_outer_islands): DiLoCo's SGD / Nesterov outer update
// taken by every node against the average of its island, each node on a master and a
// momentum row of its own, one HBM-streaming pass.  Roofline: HBM (DESIGN.md §3 "Island
// outer step").
//
// The geometry of reduce.hip: 256 threads, a workgroup owns 1024 contiguous vectors (or
// scalars) of ONE island -- blockIdx.x is the chunk, blockIdx.y the island -- so the
// reads of the three tables are workgroup-uniform.  A lane issues the loads of its
// vector from every member row back to back (the member loop unrolled, only the running
// sum kept, so an island has no size limit) and sums them in ascending member order.
// Then, for each member this process hosts (slot >= 0), it loads that member's master
// (and momentum) vector, takes the update on the shared sum and stores master, momentum
// and the member's x row through device-scope stores based at the workgroup's block of
// the row.  x may alias src (the in-place step of one process): a lane has read every
// member of its (island, vector) before its first store, the stores of a vector go to
// rows of that island only, and no two lanes share a vector of a row, so src and x
// carry no __restrict__.
//
// The element update is reduce.hip's outer_update, restated here expression for
// expression (that file is not touched, so its measured machine code stays what it is);
// tests/island_checks.py pins every rounding to the numpy oracle and the GPU tests pin
// the launch to ga_diloco_outer bit for bit.
#include "ga_common.h"

namespace ga {
namespace {

constexpr int kIslandBlock = 256;
constexpr int64_t kIslandChunk = 1024;  // vectors (or scalars) per workgroup
constexpr int64_t kMaxIslands = 65535;  // the island is gridDim.y

struct IslandParams {
    float lr, momentum, dampening, weight_decay;
    int first_step, nesterov;
};

// outer_update of reduce.hip: the same operations in the same expression shapes.
__device__ __forceinline__ float island_update(float sum, float divisor, float& master, float& buf,
                                               const IslandParams& op) {
    const float avg = sum / divisor;
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

template <typename T, bool VEC>
__global__ __launch_bounds__(kIslandBlock) void diloco_outer_islands_kernel(
    const T* src, int64_t ld_src, int64_t n, const int32_t* __restrict__ starts,
    const int32_t* __restrict__ members, const int32_t* __restrict__ slots, float* master, float* mom,
    int64_t ld_state, IslandParams op, T* x, int64_t ld_x) {
    const int32_t e0 = starts[blockIdx.y], e1 = starts[blockIdx.y + 1];
    const float divisor = (float)(e1 - e0);
    const bool has_mom = op.momentum != 0.f;
    const int64_t total = VEC ? n >> 2 : n;
    const int64_t lo = (int64_t)blockIdx.x * kIslandChunk;
    const int64_t hi = lo + kIslandChunk < total ? lo + kIslandChunk : total;
    if constexpr (VEC) {
        using V = typename Vec4<T>::type;
        for (int64_t v = lo + threadIdx.x; v < hi; v += kIslandBlock) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int32_t e = e0; e < e1; ++e) {
                float f[4];
                Vec4<T>::unpack(stream_load(reinterpret_cast<const V*>(src + (int64_t)members[e] * ld_src) + v), f);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] += f[c];
            }
            const uint32_t i = (uint32_t)(v - lo);
            for (int32_t e = e0; e < e1; ++e) {
                const int64_t slot = slots[e];
                if (slot < 0) continue;  // hosted elsewhere: summed, not updated
                float* mrow = master + slot * ld_state;
                float m[4], b[4] = {0.f, 0.f, 0.f, 0.f};
                Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(mrow) + v), m);
                if (has_mom && !op.first_step)
                    Vec4<float>::unpack(stream_load(reinterpret_cast<const float4*>(mom + slot * ld_state) + v), b);
                float out[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) out[c] = island_update(acc[c], divisor, m[c], b[c], op);
                // device-scope (sc1) stores based at the workgroup's block of each row
                store_sc1(reinterpret_cast<float4*>(mrow) + lo, i, Vec4<float>::pack(m));
                if (has_mom) store_sc1(reinterpret_cast<float4*>(mom + slot * ld_state) + lo, i, Vec4<float>::pack(b));
                store_sc1(reinterpret_cast<V*>(x + slot * ld_x) + lo, i, Vec4<T>::pack(out));
            }
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += kIslandBlock) {
            float acc = 0.f;
#pragma unroll 4
            for (int32_t e = e0; e < e1; ++e) acc += Elem<T>::load(src + (int64_t)members[e] * ld_src + i);
            for (int32_t e = e0; e < e1; ++e) {
                const int64_t slot = slots[e];
                if (slot < 0) continue;
                float* mp = master + slot * ld_state + i;
                float m = *mp;
                float b = (has_mom && !op.first_step) ? mom[slot * ld_state + i] : 0.f;
                const float out = island_update(acc, divisor, m, b, op);
                *mp = m;
                if (has_mom) mom[slot * ld_state + i] = b;
                Elem<T>::store(x + slot * ld_x + i, out);
            }
        }
    }
}

bool island_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

template <typename T>
int launch_islands(const void* src, int64_t ld_src, int64_t n, const int32_t* starts, int64_t I,
                   const int32_t* members, const int32_t* slots, float* master, float* mom, int64_t ld_state,
                   const IslandParams& op, void* x, int64_t ld_x, hipStream_t stream) {
    const int vb = 4 * (int)sizeof(T);
    const bool vec = (n % 4 == 0) && (ld_src % 4 == 0) && (ld_x % 4 == 0) && (ld_state % 4 == 0) &&
                     island_aligned(src, vb) && island_aligned(x, vb) && island_aligned(master, 16) &&
                     island_aligned(mom, 16);
    auto* kernel = vec ? diloco_outer_islands_kernel<T, true> : diloco_outer_islands_kernel<T, false>;
    const int64_t chunks = ceil_div(vec ? n / 4 : n, kIslandChunk);
    hipLaunchKernelGGL(kernel, dim3((unsigned)chunks, (unsigned)I), dim3(kIslandBlock), 0, stream, (const T*)src,
                       ld_src, n, starts, members, slots, master, mom, ld_state, op, (T*)x, ld_x);
    return check_launch("ga_diloco_outer_islands");
}

}  // namespace
}  // namespace ga

using namespace ga;

extern "C" GA_API int ga_diloco_outer_islands(int dtype, const void* src, int64_t S, int64_t ld_src, int64_t n,
                                              const int32_t* starts, int64_t I, const int32_t* members,
                                              const int32_t* slots, float* master, float* mom, int64_t K_state,
                                              int64_t ld_state, int first_step, float lr, float momentum,
                                              float dampening, float weight_decay, int nesterov, void* x,
                                              int64_t ld_x, hipStream_t stream) {
    clear_error();
    GA_REQUIRE(n >= 0 && S >= 1 && K_state >= 1, "ga_diloco_outer_islands: bad sizes n=%lld S=%lld K_state=%lld",
               (long long)n, (long long)S, (long long)K_state);
    GA_REQUIRE(I >= 1 && I <= kMaxIslands, "ga_diloco_outer_islands: %lld islands, 1 to %lld are supported",
               (long long)I, (long long)kMaxIslands);
    GA_REQUIRE(n <= (int64_t)INT32_MAX * kIslandChunk, "ga_diloco_outer_islands: n=%lld is too large", (long long)n);
    if (n == 0) return GA_OK;
    GA_REQUIRE(src && master && x, "ga_diloco_outer_islands: null src/master/x");
    GA_REQUIRE(starts && members && slots, "ga_diloco_outer_islands: null island table");
    GA_REQUIRE(momentum == 0.0f || mom, "ga_diloco_outer_islands: momentum != 0 needs a momentum buffer");
    GA_REQUIRE(S == 1 || ld_src >= n, "ga_diloco_outer_islands: ld_src < n");
    GA_REQUIRE(K_state == 1 || ld_x >= n, "ga_diloco_outer_islands: ld_x < n");
    GA_REQUIRE(K_state == 1 || ld_state >= n, "ga_diloco_outer_islands: ld_state < n");
    GA_REQUIRE(island_aligned(master, 4) && island_aligned(mom, 4),
               "ga_diloco_outer_islands: master and momentum must be 4-byte aligned");
    GA_REQUIRE(!(nesterov && (momentum <= 0.0f || dampening != 0.0f)),
               "ga_diloco_outer_islands: Nesterov momentum requires a momentum and zero dampening");
    const IslandParams op{lr, momentum, dampening, weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum == 0.0f) mom = nullptr;
    switch (dtype) {
        case GA_F32:
            return launch_islands<float>(src, ld_src, n, starts, I, members, slots, master, mom, ld_state, op, x,
                                         ld_x, stream);
        case GA_BF16:
            return launch_islands<__hip_bfloat16>(src, ld_src, n, starts, I, members, slots, master, mom, ld_state,
                                                  op, x, ld_x, stream);
        default:
            set_error("ga_diloco_outer_islands: unknown dtype %d", dtype);
            return GA_EINVAL;
    }
}
