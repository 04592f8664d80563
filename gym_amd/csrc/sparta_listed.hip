// SPARTA over index lists: the step of the two cycle selectors (ShuffledSequential,
// Partitioned: sparta.py:88-193) without a mask.  Each tensor's elements sit in an int32
// `order` arena grouped by partition (arena-global indices, redrawn once per cycle), a step
// selects one contiguous slice per participating tensor, and the host knows every slice's
// length in closed form.  The kernels walk the packed positions j < total of the step's
// table {start, count, prefix} directly: ~p n list entries read, ~p n K words touched, no
// n-element mask, no scan, no count read back.
//
// Work split (both layouts): one workgroup of 256 lanes per 256 packed positions, ONE LANE
// PER LISTED ELEMENT.  A lane finds its table row, reads e = order[start + j - prefix]
// (adjacent lanes of one tensor read adjacent entries: coalesced), then issues its replicas'
// loads back to back, up to KB words in flight per lane (KB = 8 for K <= 8, else batches of
// 32 that a K > 32 set walks in turn), sums them in ascending replica order in the lane (the
// fp32 order of ga_sparta_average_local: bit-identical), divides once and writes the average
// to every replica, or stores {e, sum} for the exchange path.  In the [K, ld] rows layout
// every (element, replica) is its own random 4-byte word, so the step is the latency of
// total x K scattered reads and writes (the floor ga_probe_random_words measures); within a
// partition the plan keeps the list ascending, so neighbouring lanes touch neighbouring DRAM
// pages of one row, as the mask kernels' ascending compaction does.
//
// Prefix table in LDS, any ntens: a 256-position tile meets at most 256 rows with count > 0,
// so the workgroup stages the WINDOW of 256 rows from the row that holds its first position
// (one uniform binary search over the table in global memory, then one row per lane), and
// each lane searches the window in LDS.  Rows with count 0 are legal (the host drops them);
// a lane whose position lies past the window then searches the table in global memory.
// Every index read from device memory is range-checked before it is used as an address.
//
// Built without packed fp32 instructions (Makefile), as topk.hip is.
#include "ga_common.h"

namespace ga {

constexpr int kLsBlock = 256;  // packed positions per workgroup, one per lane
constexpr int kLsWin = 256;    // table rows staged in LDS (>= the rows with count > 0 a tile can meet)
static_assert(kLsWin == kLsBlock, "one window row per lane");

struct ListRep {
    int64_t ek, ei;  // strides of replica and element (rows: ld, 1; element-major: 1, ld)
};

// last row t with prefix[t] <= j (rows are {start, count, prefix}; prefix[0] == 0)
__device__ __forceinline__ int list_row(const int32_t* __restrict__ tab, int ntens, int32_t j) {
    int lo = 0, hi = ntens - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[3 * mid + 2] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename T, int KB, bool GATHER>
__global__ __launch_bounds__(kLsBlock) void sparta_listed_kernel(T* reps, int K, ListRep R, int64_t n,
                                                                 const int32_t* __restrict__ order, int64_t norder,
                                                                 const int32_t* __restrict__ tab, int ntens,
                                                                 int32_t total, float divisor,
                                                                 int32_t* __restrict__ idx, T* __restrict__ vals,
                                                                 int64_t* __restrict__ count) {
    __shared__ int32_t w_start[kLsWin], w_count[kLsWin], w_prefix[kLsWin];
    const int32_t tile0 = (int32_t)blockIdx.x * kLsBlock;  // < total < 2^31
    const int t0 = list_row(tab, ntens, tile0);            // wave-uniform: scalar loads
    const int nw = ntens - t0 < kLsWin ? ntens - t0 : kLsWin;
    if ((int)threadIdx.x < nw) {
        const int32_t* row = tab + 3 * (int64_t)(t0 + (int)threadIdx.x);
        w_start[threadIdx.x] = row[0];
        w_count[threadIdx.x] = row[1];
        w_prefix[threadIdx.x] = row[2];
    }
    __syncthreads();
    if (GATHER && blockIdx.x == 0 && threadIdx.x == 0) {
        count[0] = total;
        count[1] = 0;
    }
    const int32_t j = tile0 + (int32_t)threadIdx.x;
    if (j >= total) return;
    int lo = 0, hi = nw - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (w_prefix[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    int32_t start = w_start[lo], cnt = w_count[lo], off = j - w_prefix[lo];
    if (off >= cnt) {  // past the window: the table holds rows with count 0
        const int32_t* row = tab + 3 * (int64_t)list_row(tab, ntens, j);
        start = row[0];
        cnt = row[1];
        off = j - row[2];
    }
    const int64_t slot = (int64_t)start + off;
    if (off < 0 || off >= cnt || start < 0 || slot >= norder) return;  // not a table this step can have
    const int32_t e = order[slot];
    if (e < 0 || (int64_t)e >= n) return;
    T* p = reps + (int64_t)e * R.ei;
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += KB) {
        float v[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) v[u] = k0 + u < K ? Elem<T>::load(p + (int64_t)(k0 + u) * R.ek) : 0.f;
#pragma unroll
        for (int u = 0; u < KB; ++u)
            if (k0 + u < K) acc += v[u];
    }
    if (GATHER) {
        idx[j] = e;
        Elem<T>::store(vals + j, acc);
        return;
    }
    const float avg = acc / divisor;
    for (int k = 0; k < K; ++k) Elem<T>::store(p + (int64_t)k * R.ek, avg);
}

template <typename T, bool GATHER>
static int launch_listed(void* reps, int64_t K, ListRep R, int64_t n, const int32_t* order, int64_t norder,
                         const int32_t* tab, int32_t ntens, int64_t total, float divisor, int32_t* idx, void* vals,
                         int64_t* count, hipStream_t stream, const char* what) {
    const dim3 grid((unsigned)ceil_div(total, (int64_t)kLsBlock)), block(kLsBlock);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, stream, (T*)reps, (int)K, R, n, order, norder, tab, (int)ntens,
                           (int32_t)total, divisor, idx, (T*)vals, count);
    };
    if (K <= 8) go(sparta_listed_kernel<T, 8, GATHER>);
    else go(sparta_listed_kernel<T, 32, GATHER>);
    return check_launch(what);
}

static int listed_args(const char* who, int64_t K, int64_t ld, int layout, int64_t n, int64_t norder, int32_t ntens,
                       int64_t total) {
    GA_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "%s: n=%lld out of int32 index range", who, (long long)n);
    GA_REQUIRE(K >= 1 && K < (int64_t)INT32_MAX, "%s: bad K=%lld", who, (long long)K);
    GA_REQUIRE(layout == GA_LAYOUT_ROWS || layout == GA_LAYOUT_ELEM_MAJOR, "%s: bad layout %d", who, layout);
    GA_REQUIRE(layout == GA_LAYOUT_ELEM_MAJOR ? ld >= K : (K == 1 || ld >= n), "%s: ld too small", who);
    GA_REQUIRE(ntens >= 0 && norder >= 0, "%s: bad ntens=%d norder=%lld", who, (int)ntens, (long long)norder);
    GA_REQUIRE(total >= 0 && total <= norder && total < (int64_t)INT32_MAX,
               "%s: total=%lld outside [0, norder=%lld]", who, (long long)total, (long long)norder);
    GA_REQUIRE(total == 0 || (ntens >= 1 && n >= 1), "%s: total > 0 with an empty table or arena", who);
    return GA_OK;
}

static ListRep list_rep(int64_t ld, int layout) {
    ListRep R;
    R.ek = layout == GA_LAYOUT_ELEM_MAJOR ? 1 : ld;
    R.ei = layout == GA_LAYOUT_ELEM_MAJOR ? ld : 1;
    return R;
}

}  // namespace ga

using namespace ga;

extern "C" GA_API int ga_sparta_average_listed(int dtype, void* reps, int64_t K, int64_t ld, int layout, int64_t n,
                                               const int32_t* order, int64_t norder, const int32_t* table,
                                               int32_t ntens, int64_t total, float divisor, hipStream_t stream) {
    clear_error();
    if (int e = listed_args("ga_sparta_average_listed", K, ld, layout, n, norder, ntens, total)) return e;
    GA_REQUIRE(divisor > 0.0f, "ga_sparta_average_listed: divisor must be > 0");
    if (total == 0) return GA_OK;  // an empty step launches nothing
    GA_REQUIRE(reps && order && table, "ga_sparta_average_listed: null reps/order/table");
    const char* what = "ga_sparta_average_listed";
    switch (dtype) {
        case GA_F32:
            return launch_listed<float, false>(reps, K, list_rep(ld, layout), n, order, norder, table, ntens, total,
                                               divisor, nullptr, nullptr, nullptr, stream, what);
        case GA_BF16:
            return launch_listed<__hip_bfloat16, false>(reps, K, list_rep(ld, layout), n, order, norder, table, ntens,
                                                        total, divisor, nullptr, nullptr, nullptr, stream, what);
        default: set_error("ga_sparta_average_listed: unknown dtype %d", dtype); return GA_EINVAL;
    }
}

extern "C" GA_API int ga_sparta_gather_listed(int dtype, const void* src, int64_t K, int64_t ld, int layout, int64_t n,
                                              const int32_t* order, int64_t norder, const int32_t* table,
                                              int32_t ntens, int64_t total, int32_t* idx, void* vals, int64_t* count,
                                              hipStream_t stream) {
    clear_error();
    if (int e = listed_args("ga_sparta_gather_listed", K, ld, layout, n, norder, ntens, total)) return e;
    if (total == 0) return GA_OK;  // an empty step launches nothing (count is left as it is)
    GA_REQUIRE(src && order && table && idx && vals && count, "ga_sparta_gather_listed: null buffer");
    const char* what = "ga_sparta_gather_listed";
    switch (dtype) {
        case GA_F32:
            return launch_listed<float, true>((void*)src, K, list_rep(ld, layout), n, order, norder, table, ntens,
                                              total, 1.f, idx, vals, count, stream, what);
        case GA_BF16:
            return launch_listed<__hip_bfloat16, true>((void*)src, K, list_rep(ld, layout), n, order, norder, table,
                                                       ntens, total, 1.f, idx, vals, count, stream, what);
        default: set_error("ga_sparta_gather_listed: unknown dtype %d", dtype); return GA_EINVAL;
    }
}
