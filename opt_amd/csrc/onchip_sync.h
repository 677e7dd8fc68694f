// Grid-wide hand-off primitives of the persistent ("on-chip") solver kernels: iw_onchip.h (image_warping), sfs_onchip.h, stencil_onchip.h (host side of the last two: onchip_launch.h).
//
// Everything that crosses workgroups inside such a kernel travels as naturally aligned 8-byte words {payload, tag}: ONE relaxed agent-scope store each (global_store sc1:
// written through, no fence, no cache write-back) and relaxed agent-scope loads on the polling side (MI355X_MICROARCH.md "handoff-1to1" / granule "R2"; measured in
// tools/microbench_gridsync.hip).  The tag is the iteration (phase) number, so a word says by itself whether it is the one the reader waits for; tags never repeat
// over the life of a buffer.  Every wait is bounded by the device's 100 MHz wall clock and gives up as soon as another waiter has (the `bad` word).
// The protocol of one phase of a wave-tiled kernel is here as functions: the grid-wide sum with its one bounded wait (ocGridSum), the q early-out (ocZetaBreak), alpha and
// beta from the totals (ocAlpha, ocBeta).  march_onchipPcg is built from them; sfs_onchipPcg keeps its own text of the same steps (it runs at the cap of the scalar
// registers and measurably loses with them, see sfs_onchip.h) and shares the small helpers; image_warping's kernels (two-level tree, rank hop, hand-over inside the
// workgroup) keep their own.  At the end of the file, the host side the dynamic-LDS solves of the graph kernel sets share: which variants a device offers (ocOfferable), the
// launch with the guarded update behind it (ocLaunchSolve, ocApplyDeltaToUnknowns).
#pragma once
#include "common.h"
#include <utility>

namespace optamd {

// Bounds of the waits inside a persistent kernel, in ticks of the device's 100 MHz wall clock.  `first`: the waits of the first phase -- every workgroup posts its words
// before it waits, so passing them proves the whole grid resident; a grid that is NOT co-resident (a foreign tenant holds CUs, another plan's persistent kernel) gives up
// there after 10 ms, before anything has been written, and the solver redoes the step on the streaming kernels.  `later`: once resident, a word is microseconds away; the
// bound only ends a hang (a peer that faulted) and scales with the solve: 100 ms + 100 us per PCG iteration.  Kernels whose first sum waits for OTHER PROCESSES' launches
// (row slabs: the rank hop) keep 2 s for both.  OPT_AMD_ONCHIP_TIMEOUT_MS (tests of the time-out path) overrides `later` and caps `first`.
struct OcTimeouts { long long first, later; };
inline OcTimeouts ocTimeouts(long long overrideTicks, int lIterations, bool waitsForOtherProcesses) {
    OcTimeouts t;
    t.later = waitsForOtherProcesses ? 2000LL * 100000 : (100LL + lIterations / 10) * 100000;
    t.first = waitsForOtherProcesses ? t.later : 10LL * 100000;
    if (overrideTicks > 0) { t.later = overrideTicks; t.first = std::min(t.first, overrideTicks); }
    return t;
}

// Host side of a time-out, one per kernel set with a persistent kernel (EnergyOps::onChipGuard).  A wait that gives up raises the device word `bad`; the launch's update
// kernel (or the kernel itself, where the solver applies the update) relays it to pinned host word 0 and leaves the unknowns untouched; after the stream has drained
// the solver asks failedNow(), redoes the linear solve on the streaming kernels and calls rearm() once its back-off is over.
// Switches (read once per plan): OPT_AMD_ONCHIP=0 switches the path off (the one A/B switch); OPT_AMD_ONCHIP_ROWS / _WAVES force a variant (tests run every variant on
// small images); the test hooks of the time-out path: OPT_AMD_ONCHIP_FAIL_AT=i (workgroup 0 raises `bad` in iteration i as a timed-out wait would), in the n-th on-chip
// launch of the plan only with OPT_AMD_ONCHIP_FAIL_LAUNCH=n, and OPT_AMD_ONCHIP_TIMEOUT_MS (overrides the bounds above).
struct OnchipGuard {
    bool enabled = true, failed = false, launched = false;      // failed: a wait timed out, the path is off until rearm(); launched: a launch reports to hostErr[0]
    int forceRows = 0, forceWaves = 0, failAt = -1, failLaunch = -1, launches = 0, stepSlot = -1;
    long long timeoutTicks = 0;      // 0: ocTimeouts() decides
    int* bad = nullptr;              // device word: some wait timed out
    int* hostErr = nullptr;          // pinned, 16 words: [0] a launch failed, [1 + s] the launch of deferred step s did (sticky until rearm)
    unsigned seq = 0;                // the next tag; 0: the tagged buffers have not been cleared yet
    std::vector<std::pair<void*, size_t>> tagged;
    OnchipGuard() {
        if (const char* e = getenv("OPT_AMD_ONCHIP")) enabled = atoi(e) != 0;
        if (const char* e = getenv("OPT_AMD_ONCHIP_ROWS")) forceRows = std::max(0, atoi(e));
        if (const char* e = getenv("OPT_AMD_ONCHIP_WAVES")) forceWaves = std::max(0, atoi(e));
        if (const char* e = getenv("OPT_AMD_ONCHIP_FAIL_AT")) failAt = atoi(e);
        if (const char* e = getenv("OPT_AMD_ONCHIP_FAIL_LAUNCH")) failLaunch = atoi(e);
        if (const char* e = getenv("OPT_AMD_ONCHIP_TIMEOUT_MS")) timeoutTicks = std::max(1, atoi(e)) * 100000LL;
    }
    ~OnchipGuard() {
        for (auto& b : tagged) (void)hipFree(b.first);
        if (bad) { (void)hipFree(bad); (void)hipHostFree(hostErr); }
    }
    OnchipGuard(const OnchipGuard&) = delete;
    OnchipGuard& operator=(const OnchipGuard&) = delete;
    bool usable() const { return enabled && !failed; }
    const char* whyOff() const { return !enabled ? "switched off" : failed ? "a wait timed out earlier" : nullptr; }      // (describe's why_not_on_chip)
    void allocWords(hipStream_t s) {      // (once; `bad` is cleared in stream order)
        if (bad) return;
        HIP_CHECK(hipMalloc((void**)&bad, sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&hostErr, 16 * sizeof(int))); for (int i = 0; i < 16; ++i) hostErr[i] = 0;
        HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
    }
    template <class P> P* allocTagged(size_t bytes) {      // a buffer of tagged words: cleared whenever the tags start over, freed with the guard
        void* p = nullptr; HIP_CHECK(hipMalloc(&p, bytes));
        tagged.push_back({p, bytes});
        return (P*)p;
    }
    void clearTagged(hipStream_t s) { for (auto& b : tagged) HIP_CHECK(hipMemsetAsync(b.first, 0, b.second, s)); seq = 2; }
    // The first of n fresh tags.  Zero = no tag, and tags never repeat on a buffer: the buffers are cleared before their first use and long before the counter wraps.
    unsigned tags(unsigned n, hipStream_t s) {
        if (seq == 0 || (unsigned long long)seq + n > 0xE0000000u) clearTagged(s);
        seq += n;
        return seq - n;
    }
    int failAtThisLaunch() { const int f = (failLaunch < 0 || launches == failLaunch) ? failAt : -1; ++launches; return f; }
    OcTimeouts timeouts(int L, bool crossProcess) const { return ocTimeouts(timeoutTicks, L, crossProcess); }
    // After the stream has drained: did the last launch fail?  Consumes the answer; a failure switches the path off until rearm().
    bool failedNow() {
        if (!launched) return false;
        launched = false;
        if (__atomic_load_n(hostErr, __ATOMIC_ACQUIRE) == 0) return false;
        failed = true;
        return true;
    }
    bool failedPeek() const { return launched && hostErr && __atomic_load_n(hostErr, __ATOMIC_ACQUIRE) != 0; }      // the same question, the answer not consumed
    void rearm(hipStream_t s) {      // the back-off is over: clear the failure state so that the next solve launches again (stream-ordered)
        failed = false;
        if (!bad) return;
        clearStepSlots(); __atomic_store_n(hostErr, 0, __ATOMIC_RELEASE);
        HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
    }
    // Deferred steps (PcgSolver inside Opt_ProblemSolve): the guarded update of each gets a word of its own, so that the host can tell afterwards WHICH step's solve gave up
    void setStepSlot(int slot) { stepSlot = (slot >= 0 && slot < 15) ? slot : -1; }
    int* stepWord() const { return stepSlot >= 0 ? hostErr + 1 + stepSlot : nullptr; }
    bool stepFailed(int slot) const { return hostErr && slot >= 0 && slot < 15 && __atomic_load_n(hostErr + 1 + slot, __ATOMIC_ACQUIRE) != 0; }
    void clearStepSlots() { if (hostErr) for (int i = 1; i < 16; ++i) __atomic_store_n(hostErr + i, 0, __ATOMIC_RELEASE); }
};

namespace {

typedef unsigned long long oc_u64;

// SYS: words that cross GPUs (the peer window: uncached memory, system scope); else agent scope
template <bool SYS = false> __device__ __forceinline__ oc_u64 ocLoad(const oc_u64* p) {
    return SYS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool SYS = false> __device__ __forceinline__ void ocStore(oc_u64* p, unsigned tag, unsigned half) {
    if (SYS) __hip_atomic_store(p, ((oc_u64)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else __hip_atomic_store(p, ((oc_u64)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Waits until *src carries `tag`; returns the payload.  Bounded: after timeoutTicks of the 100 MHz wall clock -- or as soon as another waiter has given up --
// the wait falls through with whatever is there (the caller's loop ends at its next sum).
template <bool SYS = false> __device__ __forceinline__ unsigned ocAwait(const oc_u64* src, unsigned tag, int* bad, long long timeoutTicks) {
    oc_u64 v = ocLoad<SYS>(src);
    if ((unsigned)(v >> 32) != tag) {
        const long long t0 = wall_clock64();
        unsigned spins = 0;
        for (;;) {
            __builtin_amdgcn_s_sleep(1);
            v = ocLoad<SYS>(src);
            if ((unsigned)(v >> 32) == tag) break;
            if ((++spins & 31u) == 0) {
                if (__hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (wall_clock64() - t0 > timeoutTicks) { __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
        }
    }
    return (unsigned)v;
}
__device__ __forceinline__ double ocJoin(unsigned lo, unsigned hi) { return __longlong_as_double((long long)(((oc_u64)hi << 32) | lo)); }

// Sum over the wave, valid in lane 63: prefix sums inside the rows of 16 lanes (row_shr 1, 2, 4, 8), then row 0 -> 1 and 2 -> 3 (row_bcast:15), then rows 0-1 -> 2-3
// (row_bcast:31).  13 DPP moves + 6 adds per double on the VALU, against six ds_bpermute round trips for the __shfl_down tree (1.2 us per iteration for four sums).
template <int CTRL, int ROWMASK> __device__ __forceinline__ double ocDppAdd(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWMASK, 0xf, true), hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWMASK, 0xf, true);
    return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ocWaveSum63(double v) {
    v = ocDppAdd<0x111, 0xf>(v); v = ocDppAdd<0x112, 0xf>(v); v = ocDppAdd<0x114, 0xf>(v); v = ocDppAdd<0x118, 0xf>(v);      // lane 15 of every row: the row's sum
    v = ocDppAdd<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = ocDppAdd<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3
    return v;
}

// ---- the one-workgroup kernels (arap_onchip.h, graph_onchip.h): one workgroup of up to 512 threads, 2 waves per SIMD, 256 registers per lane ----
constexpr int kOcWgMaxWaves = 8, kOcWgMaxBlock = kOcWgMaxWaves * kWave;
// NS sums over the workgroup, the same bits in every lane: wave sums (valid in lane 63), one partial per wave in LDS, every lane adds them in wave order.  red:
// [NS][kOcWgMaxWaves] doubles, whose entries beyond the launch's waves are zero for the life of the kernel.  One barrier; the caller passes another barrier before it
// comes back with the same `red` (the one at the top of the iteration), so the partials are not overwritten before every lane has read them.
template <int NS>
__device__ __forceinline__ void ocWorkgroupSum(double (&v)[NS], double* red, int lane, int wave, int nW) {
#pragma unroll
    for (int q = 0; q < NS; ++q) { const double s = ocWaveSum63(v[q]); if (lane == kWave - 1) red[q * kOcWgMaxWaves + wave] = s; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        double t = 0;
        for (int w = 0; w < nW; w += 2) { const double2 two = *reinterpret_cast<const double2*>(red + q * kOcWgMaxWaves + w); t += two.x; t += two.y; }
        v[q] = t;
    }
}

// one scalar as tagged words: a float is one word, a double two (ocSend); the payload of such words once they carry the tag (ocPayload)
template <bool SYS = false> __device__ __forceinline__ void ocSend(oc_u64* box, int idx, float v, unsigned tag) { ocStore<SYS>(box + idx, tag, __float_as_uint(v)); }
template <bool SYS = false> __device__ __forceinline__ void ocSend(oc_u64* box, int idx, double v, unsigned tag) {
    const oc_u64 b = (oc_u64)__double_as_longlong(v);
    ocStore<SYS>(box + 2 * idx, tag, (unsigned)b); ocStore<SYS>(box + 2 * idx + 1, tag, (unsigned)(b >> 32));
}
template <class T> __device__ __forceinline__ T ocPayload(const oc_u64* w) {
    if constexpr (sizeof(T) == 4) return __uint_as_float((unsigned)w[0]);
    else return __longlong_as_double((long long)((w[1] << 32) | (w[0] & 0xffffffffull)));
}
// lane l's v, in every lane (l: wave-uniform)
template <class T> __device__ __forceinline__ T ocReadLane(T v, int l) {
    if constexpr (sizeof(T) == 8) return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
    else return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float ocFma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double ocFma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---- The protocol of one phase of a wave-tiled kernel (march_onchipPcg).  A kernel keeps what is its own: the tile geometry, the march, which ring words a lane asks
// for, the update over the held rows.  Nothing below asks which kernel calls it: what differs is a template parameter or one of the caller's callables.

// The LDS of the grid-wide sum, declared __shared__ by the kernel.  NS: sums per phase; MAXG: workgroup cap of the family.
template <int NS, int WAVES, int MAXG>
struct OcSumLds {
    double red[NS * WAVES];       // [sum][wave]: the waves' partial sums
    double TOT[NS];               // the grid's totals: the same bits in every workgroup
    int gaveUp;                   // `bad` as thread 0 read it behind the wait: uniform over the workgroup
    unsigned W1[MAXG * 2 * NS];   // every workgroup's words, regrouped
};

// The grid-wide sum of one phase: every workgroup posts its NS partial sums as tagged words (one per half-double) into its slot of this parity, waits ONCE for all workgroups'
// words and for the ring words the kernel asks for (posted before their owners' sums), and adds all workgroups' words in workgroup order.  Afterwards S.TOT[0 .. NS - 1]
// hold the totals and S.gaveUp says whether a wait timed out somewhere (the kernel leaves its loop).  Called by every thread of the workgroup.
//   part        this lane's partial sums
//   slotPar     the parity's [G][2 NS] slot words
//   ticks       the bound of this wait (the first phase: the co-residency bound, OcTimeouts::first)
//   askRing()   request this lane's ring words into the kernel's own registers (a word that is not needed: preset to {0, tag})
//   ringHere()  do all of them carry the tag?
template <int NS, int WAVES, int MAXG, class AskRing, class RingHere>
__device__ __forceinline__ void ocGridSum(OcSumLds<NS, WAVES, MAXG>& S, const double (&part)[NS], unsigned tag, oc_u64* slotPar, int G, int* bad, long long ticks,
                                          AskRing&& askRing, RingHere&& ringHere) {
    constexpr int NW = 2 * NS, kBlk = WAVES * kWave;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = blockIdx.x;
#pragma unroll
    for (int q = 0; q < NS; ++q) { const double v = ocWaveSum63(part[q]); if (lane == kWave - 1) S.red[q * WAVES + wave] = v; }
    __syncthreads();
    if (tid < NW) {
        double s = 0;
        for (int w = 0; w < WAVES; ++w) s += S.red[(tid >> 1) * WAVES + w];
        const oc_u64 b = (oc_u64)__double_as_longlong(s);
        ocStore(slotPar + (size_t)g * NW + tid, tag, (tid & 1) ? (unsigned)(b >> 32) : (unsigned)b);
    }
    // ---- ONE wait: the ring words and every workgroup's sums are requested together, re-requested until all carry this phase's tag
    // (measured: a word-major layout that lets every wave request "its" sum directly -- no staging -- makes eight workgroups post into one 64-byte line: the wait
    //  grows from 3.5 to 5.6 us.  Workgroup-major words, thread i requests word i, the words are regrouped through LDS.)
    constexpr int kPer = (MAXG * NW + kBlk - 1) / kBlk;
    oc_u64 w[kPer];
    const int nW = G * NW;
    bool sumsOk = false, ringOk = false;
    // requests and checks apart: the first round asks for everything at once; a later round asks again only for what has not arrived (the ring words are
    // posted before their owners' sums and are normally there by then: the re-requests are the words of the sums)
    auto askSums = [&]() {
#pragma unroll
        for (int u = 0; u < kPer; ++u) { const int i = tid + u * kBlk; w[u] = ocLoad(slotPar + (i < nW ? i : tid % nW)); }
    };
    auto check = [&]() {
        if (!sumsOk) {
            bool ok = true;
#pragma unroll
            for (int u = 0; u < kPer; ++u) { const int i = tid + u * kBlk; ok = ok && (i >= nW || (unsigned)(w[u] >> 32) == tag); }
            sumsOk = ok;
        }
        if (!ringOk) ringOk = ringHere();
        return sumsOk && ringOk;
    };
    askSums(); askRing();
    if (!check()) {
        const long long t0 = wall_clock64();
        unsigned spins = 0;
        for (;;) {
            __builtin_amdgcn_s_sleep(1);
            if (!sumsOk) askSums();
            if (!ringOk) askRing();
            if (check()) break;
            if ((++spins & 31u) == 0) {
                if (__hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (wall_clock64() - t0 > ticks) { __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) { const int i = tid + u * kBlk; if (i < nW) S.W1[i] = (unsigned)w[u]; }
    __syncthreads();
    // Every workgroup adds all workgroups' words in the same order: wave q takes sum q (more sums than waves: wave 0 takes sum WAVES as well), a lane the workgroups lane,
    // lane + 64, lane + 128, lane + 192 in that order, then the wave's DPP tree -- the same association everywhere, so the same bits.
#pragma unroll
    for (int pass = 0; pass < (NS + WAVES - 1) / WAVES; ++pass) {
        const int q = wave + pass * WAVES;
        if (q < NS) {
            double sacc = 0;
#pragma unroll
            for (int c = 0; c < MAXG / kWave; ++c) {
                const int m = lane + c * kWave;
                const double v = m < G ? ocJoin(S.W1[m * NW + 2 * q], S.W1[m * NW + 2 * q + 1]) : 0.0;
                sacc += v;
            }
            sacc = ocWaveSum63(sacc);
            if (lane == kWave - 1) S.TOT[q] = sacc;
        }
    }
    if (tid == 0) S.gaveUp = __hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
}

// The q early-out (solver.t:1093-1102): zeta = mult (Q1 - Q0) / Q1 against q_tolerance.  true: break -- thread 0 of workgroup 0 leaves {reportIter, zeta} in lmBreak
// (OnChipLm::breakInfo) for a caller who listens; else Q0 = Q1.  Every workgroup decides from the same totals.
template <class T> __device__ __forceinline__ bool ocZetaBreak(T Q1, T& Q0, int mult, T qTolerance, double* lmBreak, int reportIter) {
    const T zeta = T(mult) * (Q1 - Q0) / Q1;
    if (zeta < qTolerance) {
        if (lmBreak && blockIdx.x == 0 && threadIdx.x == 0) { lmBreak[1] = (double)zeta; lmBreak[0] = (double)reportIter; }
        return true;
    }
    Q0 = Q1;
    return false;
}

// alpha and beta from the totals (the guards of solver.t:456-459, 544-547; beta's numerator by expansion, clamped like the direct sum it replaces).  rr: sum r^2 in front
// of this iteration -- alphaNum itself but for the first iteration, where the caller knows its start.
// (Two functions, so that the caller's rr is formed behind alpha as it always was: one function that returns both makes a stencil variant that sits at its register cap spill.)
template <class T> __device__ __forceinline__ T ocAlpha(double aNumD, double aDenD) {
    const T aNum = (T)aNumD, aDen = (T)aDenD;
    return (aDen > T(0)) ? aNum / aDen : T(0);
}
template <class T> __device__ __forceinline__ T ocBeta(T alpha, double aNumD, double s2, double s3, double rr) {
    const T aNum = (T)aNumD;
    const double bNumD = fmax(rr - 2.0 * (double)alpha * s2 + (double)alpha * (double)alpha * s3, 0.0);
    return (aNum > T(0)) ? (T)bNumD / aNum : T(0);
}

// PCGLinearUpdate X += delta (solver.t:552-557) behind an on-chip Gauss-Newton solve -- unless a wait timed out: then the unknowns stay untouched and the host is told
template <class T>
__global__ __launch_bounds__(kBlock) void ocApplyDelta(T* __restrict__ X, const T* __restrict__ delta, long n, const int* __restrict__ bad, int* hostErr) {
    if (__hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(hostErr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) X[i] = X[i] + delta[i];
}
// ... over every unknown image of the kernel set `ops` (EnergyOps), with at most `cap` workgroups per image
template <class T, class Ops>
void ocApplyDeltaToUnknowns(const Ops& ops, const T* delta, long cap, const OnchipGuard& guard, LaunchCtx& ctx) {
    ScopedKernel k(ctx, "PCGLinearUpdate");
    for (size_t i = 0; i < ops.unknowns.size(); ++i) {
        const auto& u = ops.unknowns[i];
        const long cnt = u.elems * u.channels;
        const int grid = (int)std::max<long>(1, std::min<long>((cnt + kBlock - 1) / kBlock, cap));
        ocApplyDelta<T><<<grid, kBlock, 0, ctx.stream>>>(ops.unknownPtr((int)i), delta + u.offset, cnt, guard.bad, guard.hostErr);
    }
}

// ---- host side of the dynamic-LDS on-chip solves of the graph kernel sets (arap_onchipPcg, ge_onchipPcg, ge_onchipPcgGrid; the wave-tiled families: onchip_launch.h) ----
// Is the variant `fn` offered on this device?  It uses no scratch (a kernel that is all latency) and the device grants it maxDynamicLdsBytes of dynamic LDS.
inline bool ocOfferable(const void* fn, size_t maxDynamicLdsBytes) {
    hipFuncAttributes fa{};
    if (fn && hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.localSizeBytes == 0 &&
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)maxDynamicLdsBytes) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
// The launch of such a solve and what follows it: behind a Gauss-Newton solve the guarded PCGLinearUpdate X += delta over the unknowns of `ops` (LM: the solver applies
// the update itself).  false: the launch was refused -- the path is switched off.
template <class T, class Ops>
bool ocLaunchSolve(const void* fn, dim3 grid, dim3 block, void** kargs, size_t ldsBytes, OnchipGuard& guard, const Ops& ops, const T* delta, bool lm, LaunchCtx& ctx) {
    guard.allocWords(ctx.stream);
    {
        ScopedKernel k(ctx, "PCGSolveOnChip");
        if (hipLaunchKernel(fn, grid, block, kargs, ldsBytes, ctx.stream) != hipSuccess) { (void)hipGetLastError(); guard.enabled = false; return false; }
    }
    if (!lm) ocApplyDeltaToUnknowns(ops, delta, 64, guard, ctx);
    guard.launched = true;
    return true;
}

}  // namespace
}  // namespace optamd
