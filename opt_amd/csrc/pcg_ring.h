// Host side of the launch-per-iteration PCG loops that keep no residual vector (stencil_march.h march_pcgIter, iw_iter.h iw_pcgIter2): p_{k-1} = M r_{k-1} +
// beta_{k-2} p_{k-2} determines r_{k-1}, so the loop state is a ring of three p buffers (p[j % 3] holds p_j) plus two ping-pong slots of alpha / beta; only the
// two launches behind a true r -- PCGInit1's, or the one a split residual reset of Levenberg-Marquardt leaves -- read the solver's residual.  delta is touched
// every second launch (two terms at once), so after an odd launch one term is owed.  This file is the one place that knows which buffer and which slot a launch uses.
#pragma once
#include "common.h"

namespace optamd {
namespace {

// delta += alpha[0] * p over n scalars: the term a deferring launch left owed (alpha as that launch wrote it)
template <class T>
__global__ __launch_bounds__(kBlock) void axpyDeferred(T* __restrict__ delta, const T* __restrict__ p, const T* __restrict__ alpha, long n) {
    const T a = alpha[0];
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) delta[i] += a * p[i];
}

template <class T>
struct PcgRing {
    struct Launch {                        // what launch k reads and writes
        int k, flip;                       // launch number within the linear solve; sweep direction (0 top-down)
        const T *pOld, *rOld; T* pNew;     // p_{k-1};  rfree == 2: the true r, rfree == 1: p_{k-2};  p_k
        int rfree;
        int deltaMode;                     // 2: this launch leaves delta alone;  1: it applies alpha_{k-2} p_{k-2} + alpha_{k-1} p_{k-1}
        const T* alphaIn; T* alphaOut;     // alpha, beta the previous launch left ([0], [2]) / where this launch leaves its own
        const T* owedP;                    // != nullptr: this launch deferred alpha_{k-1} p_{k-1} (= alphaOut[0] * owedP)
    };
    T* p[3] = {nullptr, nullptr, nullptr}; T* alphaSlots = nullptr;      // alphaSlots: [0,1] alpha, [2,3] beta, ping-pong
    const T* r0 = nullptr;                 // the solver swaps its r buffers after every launch; the ring keeps the true r until the second launch behind it has read it
    int iterIndex = 0, sinceTrueR = 0, flip = 0; bool owed = false;
    ~PcgRing() { for (T* b : p) if (b) (void)hipFree(b); if (alphaSlots) (void)hipFree(alphaSlots); }
    void allocate(size_t nScalars, hipStream_t stream) {
        const size_t bytes = (nScalars + 3) / 4 * 4 * sizeof(T);      // padded like the solver's vectors: its flat kernels read whole 16-byte packs of the last p
        for (T*& b : p) if (!b) { HIP_CHECK(hipMalloc((void**)&b, bytes)); HIP_CHECK(hipMemsetAsync(b, 0, bytes, stream)); }
        if (!alphaSlots) { HIP_CHECK(hipMalloc((void**)&alphaSlots, 4 * sizeof(T))); HIP_CHECK(hipMemsetAsync(alphaSlots, 0, 4 * sizeof(T), stream)); }
    }
    // Successive launches sweep top-down / bottom-up, so that a launch starts on the rows the previous one left in the caches; every linear solve starts top-down,
    // so a solve is reproducible whatever ran before it.  (next() calls it; a loop that keeps its vectors in the solver's buffers takes only this.)
    int nextSweep(bool first) { if (first) flip = 0; const int f = flip; flip ^= 1; return f; }
    // The state of the next launch.  first: the launch behind PCGInit1 (rOld = r_0, pOld = p_0);  afterReset: the one behind a residual reset (rOld = the fresh r)
    Launch next(bool first, bool afterReset, const T* rOld, const T* pOld) {
        if (first) iterIndex = 0;
        if (first || afterReset) { r0 = rOld; sinceTrueR = 0; }
        const int k = iterIndex++, since = sinceTrueR++;
        Launch L{};
        L.k = k; L.flip = nextSweep(first);
        L.pOld = k == 0 ? pOld : p[(k - 1) % 3];
        L.rOld = since <= 1 ? r0 : p[(k - 2) % 3];
        L.pNew = p[k % 3];
        L.rfree = since <= 1 ? 2 : 1;
        L.deltaMode = (since >= 2 && since % 2 == 0) ? 1 : 2;      // the launch behind a true r has nothing to apply; odd launches defer
        L.alphaOut = alphaSlot(k); L.alphaIn = alphaSlot(k + 1);
        owed = since % 2 == 1;
        L.owedP = owed ? L.pOld : nullptr;
        return L;
    }
    T* alphaSlot(int j) const { return alphaSlots + (j & 1); }                                   // of launch j
    const T* pLast() const { return iterIndex >= 1 ? p[(iterIndex - 1) % 3] : nullptr; }         // p of the last launch
    const T* pPrev() const { return iterIndex >= 2 ? p[(iterIndex - 2) % 3] : nullptr; }         // ... and of the one before
    bool termOwed() const { return owed && iterIndex >= 2; }                                     // alphaSlot(iterIndex - 1)[0] * pPrev() is still to be added to delta
    void settled() { owed = false; }                                                             // (someone added it in a pass of their own)
    // After the last launch of a linear solve: adds the owed term, if any; returns where the last p lives (the solver adds the last alpha p)
    const T* finish(T* delta, long n, int grid, LaunchCtx& ctx) {
        if (termOwed()) {
            ScopedKernel sk(ctx, "PCGStep2_delta");
            axpyDeferred<T><<<grid, kBlock, 0, ctx.stream>>>(delta, pPrev(), alphaSlot(iterIndex - 1), n);
        }
        owed = false;
        return pLast();
    }
};

}  // namespace
}  // namespace optamd
