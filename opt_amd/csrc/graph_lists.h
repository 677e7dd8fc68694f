// The edge lists of a vertex, built once: for every vertex the ids j * nE + e of the (hyperedge e, slot j) pairs it occupies, ascending, as CSR (off, idx) -- the
// fixed summation order of every gather of the graph kernel sets.  GraphOps (graph_engine.h) keeps one list over its functor's V slots; ArapOps (energy_graph.hip) two
// one-slot lists, out = {v0} and in = {v1}, whose ids are therefore edge ids, behind ONE change decision over both arrays.
// A list is rebuilt when the graph arrays change: their pointers, the counts, or an order-dependent checksum of their contents (computed on the device and read back:
// the one synchronisation of a bind).  The rebuild is a counting sort: count -> exclusive scan -> fill -> per-vertex insertion sort.
// Everything here sits in this file's unnamed namespace, like graph_pcg.h's types: a plug-in that compiles this header into its own shared object runs its own copy.
#pragma once
#include "graph_common.h"
#include <hipcub/hipcub.hpp>

namespace optamd {
namespace {

template <int V> struct SlotIdx { const int* p[V]; };

template <int V>
__global__ __launch_bounds__(kBlock) void inc_checksum(SlotIdx<V> vi, int nE, unsigned long long* __restrict__ out) {
    unsigned long long acc = 0;      // integer sum: order-independent
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nE; e += gridDim.x * blockDim.x)
#pragma unroll
        for (int j = 0; j < V; ++j) acc += ((unsigned long long)(unsigned)vi.p[j][e] * 0x9E3779B97F4A7C15ull) ^ ((unsigned long long)(j * (long)nE + e) * 0x165667B19E3779F9ull);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, kWave);
    __shared__ unsigned long long part[kBlock / kWave];      // one atomic per workgroup: 12 000 wave-level atomics on one address took 100 us per bind
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long t = 0; for (int w = 0; w < kBlock / kWave; ++w) t += part[w]; atomicAdd(out, t); }
}
template <int V>
__global__ __launch_bounds__(kBlock) void inc_count(SlotIdx<V> vi, int nE, int* __restrict__ deg) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nE; e += gridDim.x * blockDim.x)
#pragma unroll
        for (int j = 0; j < V; ++j) atomicAdd(deg + vi.p[j][e], 1);
}
template <int V>
__global__ __launch_bounds__(kBlock) void inc_fill(SlotIdx<V> vi, int nE, const int* __restrict__ off, int* __restrict__ cur, int* __restrict__ idx) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nE; e += gridDim.x * blockDim.x)
#pragma unroll
        for (int j = 0; j < V; ++j) { const int v = vi.p[j][e]; idx[off[v] + atomicAdd(cur + v, 1)] = j * nE + e; }
}
__global__ __launch_bounds__(kBlock) void inc_sort(long N, const int* __restrict__ off, int* __restrict__ idx) {   // per-vertex insertion sort: fixed summation order
    for (long v = blockIdx.x * (long)blockDim.x + threadIdx.x; v < N; v += (long)gridDim.x * blockDim.x) {
        const int b = off[v], e = off[v + 1];
        for (int i = b + 1; i < e; ++i) { const int x = idx[i]; int j = i - 1; while (j >= b && idx[j] > x) { idx[j + 1] = idx[j]; --j; } idx[j + 1] = x; }
    }
}

struct VertexLists {
    static constexpr int kMaxSlots = 4;
    DevBuf<int> off, idx, cur;      // [N + 1] offsets, [max(1, nE) V] ids, [N + 1] degrees, then fill cursors
    DevBuf<char> scanTemp;
    DevBuf<unsigned long long> dSum;
    const int* sigP[kMaxSlots] = {}; int sigNE = -1; long sigN = -1; unsigned long long sigSum = 0; bool valid = false;      // what the lists were built from

    // count -> scan -> fill -> sort, unconditionally, on the stream
    template <int V>
    void build(SlotIdx<V> s, int nE, long N, int cus, hipStream_t st) {
        const size_t nv = (size_t)N + 1;
        off.reserve(nv); cur.reserve(nv); idx.reserve((size_t)std::max(1, nE) * V);
        const int ge = edgeGrid(nE, cus);
        HIP_CHECK(hipMemsetAsync(cur, 0, nv * 4, st));
        inc_count<V><<<ge, kBlock, 0, st>>>(s, nE, cur);
        size_t need = 0;
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, cur.p, off.p, (int)nv, st));
        scanTemp.reserve(need);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(scanTemp.p, need, cur.p, off.p, (int)nv, st));
        HIP_CHECK(hipMemsetAsync(cur, 0, nv * 4, st));
        inc_fill<V><<<ge, kBlock, 0, st>>>(s, nE, off, cur, idx);
        inc_sort<<<(int)std::max<long>(1, std::min<long>((N + kBlock - 1) / kBlock, kMaxPartials / 2)), kBlock, 0, st>>>(N, off, idx);
    }
    // The change decision over the slots `s`, and rebuild() under the timer name if they changed (true).  The checksum's read-back is the one synchronisation.
    template <int V, class Rebuild>
    bool ensureBy(SlotIdx<V> s, int nE, long N, int cus, LaunchCtx& ctx, const char* timerName, Rebuild&& rebuild) {
        static_assert(V <= kMaxSlots, "signature slots");
        hipStream_t st = ctx.stream;
        dSum.reserve(1);
        HIP_CHECK(hipMemsetAsync(dSum, 0, 8, st));
        inc_checksum<V><<<edgeGrid(nE, cus), kBlock, 0, st>>>(s, nE, dSum);
        unsigned long long sum = 0;
        HIP_CHECK(hipMemcpyAsync(&sum, dSum, 8, hipMemcpyDeviceToHost, st)); HIP_CHECK(hipStreamSynchronize(st));
        bool same = valid && sigNE == nE && sigN == N && sigSum == sum;
        for (int j = 0; j < V; ++j) same = same && sigP[j] == s.p[j];
        if (same) return false;
        ScopedKernel k(ctx, timerName);
        rebuild();
        for (int j = 0; j < V; ++j) sigP[j] = s.p[j];
        sigNE = nE; sigN = N; sigSum = sum; valid = true;
        return true;
    }
    template <int V>
    bool ensure(SlotIdx<V> s, int nE, long N, int cus, LaunchCtx& ctx, const char* timerName) {      // true: rebuilt
        return ensureBy(s, nE, N, cus, ctx, timerName, [&] { build(s, nE, N, cus, ctx.stream); });
    }
};

}  // namespace
}  // namespace optamd
