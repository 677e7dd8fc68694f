// Gauss-Newton / Levenberg-Marquardt outer loop + matrix-free PCG inner loop, generic over the energy.
//
// What it reproduces (reference API/src/solverGPUGaussNewton.t): init :956-1007, step :1016-1177 with the
// same kernel order, the same guards (alpha = 0 unless denominator > 0 :456-459, beta :544-547), the CERES
// guarded inverse :323-332, the LM diagonal / trust-region logic :631-664, 1119-1157, the residual reset
// every `residual_reset_period` iterations :1077-1086 and the q-based early out :1093-1102.
// What it changes (MI355X-first):
//  * the streaming kernels (Step2, Step3, LinearUpdate, ...) run over the FLAT unknown vector with 16-byte
//    accesses -- they never touch the exclude mask (see energy.h contract);
//  * global sums are per-workgroup partials in double, summed in index order by each consumer workgroup:
//    no same-address atomics, no hipMemset/hipMemcpy between kernels, bitwise reproducible;
//  * alphaNumerator <- betaNumerator (a D2D memcpy per iteration in the reference, :1091) is a two-slot
//    rotation written by workgroup 0 of Step3.
#include "solver.h"
#include "onchip_sync.h"
#include "pcg_flat_kernels.h"
#include <chrono>
#include <mutex>
#include <cmath>
#include <cstddef>
#include <cstring>

// a polite spin: pause on x86, yield on arm64, nothing elsewhere
static inline void cpuRelax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#endif
}

namespace optamd {

// ------------------------------------------------------------------------------------------------------
template <class T>
struct PcgSolver : SolverBase {
    std::unique_ptr<EnergyOps<T>> E;
    bool lm;
    bool patch = false; int patchSweep = 0;   // kind "patchGaussNewtonGPU": block-local sweeps instead of the global PCG loop (stepPatch)
    hipStream_t stream = nullptr;
    LaunchCtx ctx;
    long n = 0, nPad = 0, nPacks = 0;
    int streamGrid = 0;
    // PlanData vectors (solver.t:173-185); LM-only ones are allocated for LM plans only; `g` is never used by the reference
    T *delta = nullptr, *r = nullptr, *b = nullptr, *Adelta = nullptr, *z = nullptr, *p = nullptr, *Ap_X = nullptr, *CtC = nullptr, *preconditioner = nullptr,
      *SSq = nullptr, *prevX = nullptr;
    T* p2 = nullptr;                    // second search-direction buffer for the fused PCGStep3+PCGStep1 kernel
    T *r2 = nullptr, *Ap2 = nullptr;    // second r / Ap buffers for the single-kernel PCG iteration (z doubles as nothing there)
    T* delta2 = nullptr;                // second delta buffer of the LM single-kernel loop (allocated on first use)
    bool oneKernel = true;              // OPT_AMD_ONEKERNEL=0: use the Step1(+3)/Step2 pair instead of one kernel per PCG iteration
    bool oneKernelLM = true;            // OPT_AMD_ONEKERNEL_LM=0: the same switch for the Levenberg-Marquardt loop only
    Reduction setS[2][4];               // ping-pong {alphaNum, alphaDen, s2, s3} of the single-kernel iteration
    // What a linear solve reports (solveLinear and the paths it tries).  none: the path did not run (of solveLinear: a redo stopped short of the reference-order loop).
    enum class Path { none, onChip, perIteration, referenceOrder };
    struct Solved {
        Path path = Path::none;
        bool updated = false;           // this step's PCGLinearUpdate was folded into the end of the PCG loop (EnergyOps::finishUpdate, the on-chip Gauss-Newton kernels)
        explicit operator bool() const { return path != Path::none; }
        bool onChip() const { return path == Path::onChip; }
    };
    std::vector<void*> allocs;          // device memory (allocVec, allocRed)
    std::vector<void*> pinned;          // pinned host memory (allocPinned)
    Reduction redA, redB, redQ, redC;   // alpha denominator, beta numerator, q, cost / init numerator
    Reduction redQ2;                    // second Q buffer: the LM single-kernel loop enqueues launch k + 1 (which writes Q_k) before the host has read Q_{k-1}
    Reduction redQR;                    // pinned: Q of the split residual reset (its own buffer: the reset is enqueued while the host may still poll redQ / redQ2)
    unsigned long long* stampFlag = nullptr; unsigned long long stampSeq = 0; bool pollSync = true;   // drain(): false (only after a stamp failed to arrive) -> hipStreamSynchronize
    Reduction redMH, redCH;             // pinned: model cost / cost partials that only the host sums (no copy kernel between the producer and the read)
    unsigned launchTag = 0;             // tags of the Q partials the single-kernel LM launches deliver as self-validating words (common.h storeTaggedPartial)
    bool taggedQ = true;                // Q of the single-kernel LM launches as tagged words the host polls; false (only after a tag failed to arrive): plain partials + an event in the stream
    double* scal = nullptr;             // device: [0],[1] alphaNumerator ping-pong, [2..5] slab totals
    double* scal4[2] = {nullptr, nullptr};   // device: all-reduced {alphaNum, alphaDen, s2, s3} of the single-kernel iteration (slab mode), ping-pong
    int aSlot = 0;
    double* hostBuf = nullptr;          // pinned
    double* hostBufQ = nullptr; hipEvent_t qEvent = nullptr; int qCount = 0; const double* qSrc = nullptr;   // pinned buffer + event of the overlapped q fetch
    T prevCost = 0;
    T trust_region_radius = 0, radius_decrease_factor = 0, min_lm_diagonal = 0, max_lm_diagonal = 0;   // pd.parameters (o.t:933-938)
    hipEvent_t overallStart = nullptr; bool overallOpen = false;
    OptAmd_SlabComm comm{};
    OptAmd_SlabCommExt commExt{};       // the communicator's optional fast paths (OptAmd_PlanSetSlabExt); all null unless set
    bool distributed = false;

    T* allocVec() {
        T* v; HIP_CHECK(hipMalloc((void**)&v, nPad * sizeof(T))); HIP_CHECK(hipMemset(v, 0, nPad * sizeof(T)));   // zero-initialised like o.t:627-632
        allocs.push_back(v); return v;
    }
    Reduction allocRed() {
        Reduction R; HIP_CHECK(hipMalloc((void**)&R.partials, kMaxPartials * sizeof(double))); HIP_CHECK(hipMemset(R.partials, 0, kMaxPartials * sizeof(double)));
        allocs.push_back(R.partials); return R;
    }
    void* allocPinned(size_t bytes) {
        void* v; HIP_CHECK(hipHostMalloc(&v, bytes));
        pinned.push_back(v); return v;
    }
    PcgSolver(EnergyOps<T>* e, bool useLM, bool timing, int verb) : E(e), lm(useLM) {
        verbosity = verb; timer.enabled = timing;
        HIP_CHECK(hipStreamCreate(&stream));   // blocking stream: ordered against the caller's null-stream work
        ctx.stream = stream; ctx.timer = timing ? &timer : nullptr;
        n = E->nScalars; nPad = (n + 3) / 4 * 4; nPacks = nPad / PackN<T>::N;
        int dev = 0, cus = 256; HIP_CHECK(hipGetDevice(&dev));
        HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        streamGrid = flatGrid(nPacks, cus, kMaxPartials);
        delta = allocVec(); r = allocVec(); z = allocVec(); p = allocVec(); Ap_X = allocVec(); CtC = allocVec(); preconditioner = allocVec();
        if (lm) { b = allocVec(); Adelta = allocVec(); SSq = allocVec(); prevX = allocVec(); }
        p2 = allocVec();
        if (const char* e = getenv("OPT_AMD_ONEKERNEL")) oneKernel = atoi(e) != 0;
        if (const char* e = getenv("OPT_AMD_ONEKERNEL_LM")) oneKernelLM = atoi(e) != 0;
        r2 = allocVec(); Ap2 = allocVec();                // second r / A p buffers of the single-kernel iterations (kernels that keep A p in memory read the old one on a halo)
        for (auto& st : setS) for (auto& R : st) R = allocRed();
        redA = allocRed(); redB = allocRed(); redC = allocRed();
        // Q (solver.t:483-485, 1093-1102) is read by the host once per LM iteration and by no kernel: its partials go straight to pinned host memory
        // (<= 16 KB of posted writes per launch) instead of through a device buffer and a copy kernel per iteration (830 copyBuffer launches, 7 % of config 3's GPU time)
        // With the single-kernel loop each partial is two tagged words (2 x kMaxPartials slots), which the host polls: no event packet in the stream either.
        for (Reduction* R : {&redQ, &redQ2, &redQR, &redMH, &redCH}) { R->partials = (double*)allocPinned(2 * kMaxPartials * sizeof(double)); memset(R->partials, 0, 2 * kMaxPartials * sizeof(double)); R->hostVisible = true; }
        stampFlag = (unsigned long long*)allocPinned(64); *stampFlag = 0;
        HIP_CHECK(hipMalloc((void**)&scal, 16 * sizeof(double))); HIP_CHECK(hipMemset(scal, 0, 16 * sizeof(double))); allocs.push_back(scal);
        scal4[0] = scal + 8; scal4[1] = scal + 12;
        hostBuf = (double*)allocPinned(2 * kMaxPartials * sizeof(double));      // room for two reductions read in one go (LM: model cost + new cost)
        E->slab = Slab{};
        chip = E->onChipGuard();
        hipDevice_t streamDev = 0; HIP_CHECK(hipStreamGetDevice(stream, &streamDev));
        static std::timed_mutex leases[64];
        lease = &leases[(unsigned)streamDev % 64u];
    }
    ~PcgSolver() override {
        (void)hipStreamSynchronize(stream);
        dropLease();
        for (void* a : allocs) (void)hipFree(a);
        for (void* a : pinned) (void)hipHostFree(a);
        if (onChipTrace) (void)hipFree(onChipTrace);
        deltaTrial.destroyEvents();
        if (qEvent) (void)hipEventDestroy(qEvent);
        (void)hipStreamDestroy(stream);
    }

    // ---- co-residency of the persistent kernels (EnergyOps::pcgSolveOnChip): their workgroups wait for each other, so the whole grid has to be resident ----
    // (i)  Two plans of ONE process stepped from two host threads would interleave two such grids on the CUs: a process-wide lease per device serialises the
    //      on-chip launches -- taken before the launch, dropped when this step has drained the stream; a plan that cannot get it within 50 ms runs this step
    //      on the streaming kernels.
    // (ii) A foreign tenant (another process, another library's long kernel) is caught by the kernel itself: the waits of its FIRST phase are bounded by
    //      10 ms (firstTicks) -- every workgroup posts its words before it waits, so passing that wait proves the grid resident; nothing has been written by then.
    // (iii) After a time-out the step is redone by the streaming kernels and the plan stays on them for `onChipBackoff` clean steps (8, then 16, 32 ... 1024), then
    //      tries the chip again (OnchipGuard::rearm): a tenant that has left does not cost the plan its fast path for life.
    // The lease is the mutex of the device the plan's stream was created on, resolved once in the constructor (the caller may switch devices between a step's lock and
    // its unlock).  Inside Opt_ProblemSolve it is held across the deferred steps until they are settled.
    std::timed_mutex* lease = nullptr;
    bool leaseHeld = false;
    bool takeLease() { if (leaseHeld) return true; leaseHeld = lease->try_lock_for(std::chrono::milliseconds(50)); return leaseHeld; }
    void dropLease() { if (leaseHeld) { lease->unlock(); leaseHeld = false; } }
    OnchipGuard* chip = nullptr;      // the kernel set's on-chip time-out protocol (EnergyOps::onChipGuard), or nullptr: the plan never runs on chip
    int onChipFailures = 0, onChipBackoff = 0, onChipCleanSteps = 0;
    bool onChipOff() const { return chip && chip->failed; }      // a wait timed out: the plan is on the streaming kernels until the back-off is over
    // An on-chip solve gave up (its failure word consumed): count it, set the back-off, say so (the first three times) -- `redo` is what happens to the step.
    void onChipFailure(const char* redo) {
        dropLease();      // the launch has left the chip
        chip->failed = true;
        ++onChipFailures; onChipCleanSteps = 0; onChipBackoff = std::min(8 << std::min(onChipFailures - 1, 7), 1024);
        if (onChipFailures <= 3)
            fprintf(stderr, "Opt(amd): a wait inside the on-chip PCG kernel timed out (its workgroups were not co-resident: is the GPU shared?); %s "
                            "with the streaming kernels and the plan stays on them for %d steps before it tries the chip again\n", redo, onChipBackoff);
    }
    // a step on the streaming kernels has ended: the back-off is over after onChipBackoff of them, and the next step tries the chip again
    void onChipCleanStep() {
        if (onChipOff() && ++onChipCleanSteps >= onChipBackoff) chip->rearm(stream);
    }
    bool boundForSolve = false;      // bind() has run inside the current Opt_ProblemSolve (SolverBase::insideSolve)
    bool boundOncePerSolve() const { return insideSolve && boundForSolve && E->bindInvariantDuringSolve(); }      // nothing bind() derives can have changed since init()'s
    bool gnInitByKernelSet() const { return !lm && !distributed && singleKernelAllowed() && sp.lIterations > 0; }   // PCGInit1 may be the kernel set's own pass (evalJTFInit, evalCostAndJTFInit)
    bool jtfReady = false;           // the pass that computed the last step's cost also ran this step's PCGInit1 (EnergyOps::evalCostAndJTFInit; only inside Opt_ProblemSolve)
    // Where delta lives (round 6).  delta is the one vector the Gauss-Newton loop reads AND writes, and the time of a launch follows the region the allocator put it in
    // (profiles/NOTES.md: 173 / 176 / 191 us at 4096^2 for the same binary in one process, region by region; the ring, the flag bytes and the caller's arrays do not matter).
    // The first long linear solve of a large single-GPU plan therefore tries kCands allocations of it: after launch kFirst delta is copied into a fresh vector
    // every kWindow launches (a copy: no bit changes), each window is timed with one event pair, the loop goes on in the fastest and the others are freed.
    // OPT_AMD_DELTA_TRIAL=0: off, 2: report on stderr.
    struct DeltaTrial {
        static constexpr int kCands = 4, kWindow = 6, kFirst = 4;
        int mode = 1, phase = 0, attempts = 0; std::vector<T*> vecs; std::vector<float> ms; hipEvent_t ev[2] = {nullptr, nullptr};
        DeltaTrial() { if (const char* e = getenv("OPT_AMD_DELTA_TRIAL")) mode = atoi(e); }
        void destroyEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }      // (from ~PcgSolver, before the stream goes)
        static bool applies(const PcgSolver& s) { return !s.lm && !s.distributed && s.E->deltaMovable() && s.nPad * sizeof(T) >= ((size_t)64 << 20); }
        void drop(PcgSolver& s, T* keep) {      // free every trial vector but `keep`
            for (T* v : vecs) if (v != keep) { for (auto it = s.allocs.begin(); it != s.allocs.end(); ++it) if (*it == (void*)v) { s.allocs.erase(it); break; } (void)hipFree(v); }
            vecs.clear(); ms.clear();
        }
        // before launch lIter of the launch-per-iteration Gauss-Newton loop: may move s.delta
        void beforeLaunch(PcgSolver& s, int lIter) {
            if (s.traceEnabled || !mode || phase == 2 || !applies(s)) return;
            if (lIter == 0) {
                if (phase == 1) { drop(s, s.delta); phase = 0; }      // the last solve ended inside the trial: it stayed where it had got to
                if (phase == 0 && attempts < 2 && s.sp.lIterations > kFirst + kCands * kWindow) { phase = 1; ++attempts; vecs.assign(1, s.delta); ms.clear(); }
            }
            if (phase != 1 || lIter < kFirst || (lIter - kFirst) % kWindow != 0) return;
            const int w = (lIter - kFirst) / kWindow;      // the window about to start
            if (!ev[0]) { HIP_CHECK(hipEventCreate(&ev[0])); HIP_CHECK(hipEventCreate(&ev[1])); }
            if (w > 0) {
                float t = 0;
                HIP_CHECK(hipEventRecord(ev[1], s.stream)); HIP_CHECK(hipEventSynchronize(ev[1])); HIP_CHECK(hipEventElapsedTime(&t, ev[0], ev[1]));
                ms.push_back(t);
            }
            auto moveTo = [&](T* to) { if (to != s.delta) { HIP_CHECK(hipMemcpyAsync(to, s.delta, s.nPad * sizeof(T), hipMemcpyDeviceToDevice, s.stream)); s.delta = to; } };
            if (w == 0) { HIP_CHECK(hipEventRecord(ev[0], s.stream)); return; }
            if (w < kCands) {
                T* v = nullptr;
                if (hipMalloc((void**)&v, s.nPad * sizeof(T)) == hipSuccess) {
                    s.allocs.push_back(v); vecs.push_back(v);
                    moveTo(v);
                    HIP_CHECK(hipEventRecord(ev[0], s.stream));
                    return;
                }
                (void)hipGetLastError();      // (no room for another: decide among those timed so far)
            }
            int best = 0;
            for (int i = 1; i < (int)ms.size(); ++i) if (ms[i] < ms[best]) best = i;
            if (mode > 1) { fprintf(stderr, "Opt(amd): delta placement trial, ms per %d launches:", kWindow); for (float m : ms) fprintf(stderr, " %.3f", m); fprintf(stderr, " -> %d\n", best); }
            moveTo(vecs[(size_t)best]);
            HIP_CHECK(hipStreamSynchronize(s.stream));      // (the copy out of a vector about to be freed has finished)
            drop(s, s.delta);
            phase = 2;
        }
        std::string describe(const PcgSolver& s) const {
            if (!applies(s)) return "";
            return std::string("; delta_placement_trial=") + (!mode ? "off" : phase == 2 ? "done" : phase == 1 ? "running" : "before the first linear solve of more than 28 launches");
        }
    };
    DeltaTrial deltaTrial;
    // Deferred Gauss-Newton steps (inside Opt_ProblemSolve, kernel sets with evalCostAndJTFInit): nothing a step computes steers the next one -- the cost is only reported --
    // so up to kDefer - 1 steps are enqueued back to back and their costs (one pinned partials buffer each) and on-chip verdicts (one word each) are read at the next drain.
    static constexpr int kDefer = 8;
    struct PendingStep { int slot, step; bool onChip; };
    std::vector<PendingStep> pendingSteps;
    Reduction costRing[kDefer];
    bool onChipAllowed() const { return !onChipOff() && sp.amd_onchip != 0 && sp.amd_reference_order == 0; }
    bool singleKernelAllowed() const { return oneKernel && sp.amd_reference_order == 0; }
    double* lmBreak = nullptr;          // pinned: {iteration + 1, zeta} of an on-chip LM solve's q early-out (OnChipLm::breakInfo)
    bool lastStepOnChip = false; double* onChipTrace = nullptr; int onChipTraceCap = 0;      // EnergyOps::pcgSolveOnChip
    // true iff `mine` holds on every rank: one all-reduce of a count and one read-back (once per Gauss-Newton step in slab mode)
    bool allRanksAgree(bool mine) {
        hostBuf[0] = mine ? 0.0 : 1.0;
        HIP_CHECK(hipMemcpyAsync(scal + 5, hostBuf, sizeof(double), hipMemcpyHostToDevice, stream));
        comm.allReduceSum(comm.ctx, scal + 5, 1, (void*)stream);
        return readBack(scal + 5, 1)[0] == 0.0;
    }
    // ---- reductions ---------------------------------------------------------------------------------
    // n doubles of device memory on the host (blocking D2H like the reference's computeCost / fetchQ, solver.t:790-814): valid until the next readBack
    const double* readBack(const double* dev, int n) {
        HIP_CHECK(hipMemcpyAsync(hostBuf, dev, n * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return hostBuf;
    }
    static double sumOf(const double* v, int n) { double s = 0; for (int i = 0; i < n; ++i) s += v[i]; return s; }      // in index order, like every device consumer
    // Host value of a reduction
    double hostSum(const Reduction& R) {
        if (distributed) { reduceAcross(&R, 1, scal + 2); return readBack(scal + 2, 1)[0]; }
        if (R.hostVisible) { drain(); return sumOf(R.partials, R.n); }
        return sumOf(readBack(R.partials, R.n), R.n);
    }
    // The same value without draining the stream: begin enqueues the copy and an event, end waits for that event only.
    void beginHostSum(const Reduction& R) {
        if (!hostBufQ) { hostBufQ = (double*)allocPinned(kMaxPartials * sizeof(double)); HIP_CHECK(hipEventCreateWithFlags(&qEvent, hipEventDisableTiming)); }
        if (distributed) {
            reduceAcross(&R, 1, scal + 2);
            HIP_CHECK(hipMemcpyAsync(hostBufQ, scal + 2, sizeof(double), hipMemcpyDeviceToHost, stream));
            qCount = 1;
            qSrc = hostBufQ;
        } else if (R.hostVisible) {
            qSrc = R.partials; qCount = R.n;      // the producer wrote pinned host memory: the event is all that is needed
        } else {
            HIP_CHECK(hipMemcpyAsync(hostBufQ, R.partials, R.n * sizeof(double), hipMemcpyDeviceToHost, stream));
            qCount = R.n; qSrc = hostBufQ;
        }
        HIP_CHECK(hipEventRecord(qEvent, stream));
    }
    double endHostSum() {
        HIP_CHECK(hipEventSynchronize(qEvent));
        return sumOf(qSrc, qCount);
    }
    // Spin on pinned memory until arrived() holds.  The stream is queried now and then so that a faulted or never-issued producer ends in the caller's message
    // instead of a hang: if it reports idle and the value has not been seen, fall back to the runtime's own completion (which also makes the device's writes
    // to pinned memory visible) and look once more.  false: still missing then.
    template <class Arrived> bool spinUntil(Arrived arrived) {
        for (unsigned long spins = 1; !arrived(); ++spins) {
            if ((spins & 0x3fff) == 0) {
                const hipError_t e = hipStreamQuery(stream);
                if (e != hipSuccess && e != hipErrorNotReady) HIP_CHECK(e);
                if (e == hipSuccess) { HIP_CHECK(hipStreamSynchronize(stream)); return arrived(); }
            }
            cpuRelax();
        }
        return true;
    }
    // Everything enqueued so far has finished and what it wrote to pinned memory is readable.  A one-thread kernel stamps a pinned word and the host spins
    // on it: no barrier packet with a completion signal in the queue and no wake-up through the runtime (the latency-bound LM steps drain twice or more).
    void drain() {
        if (!pollSync) { HIP_CHECK(hipStreamSynchronize(stream)); return; }
        const unsigned long long v = ++stampSeq;
        k_stamp<<<1, kWave, 0, stream>>>(stampFlag, v);
        if (!spinUntil([&] { return __atomic_load_n(stampFlag, __ATOMIC_ACQUIRE) == v; })) {      // polling is given up for this plan rather than the process
            fprintf(stderr, "Opt(amd): completion stamp %llu not visible after a stream synchronise; switching this plan to hipStreamSynchronize\n", v);
            pollSync = false;
        }
    }
    // Sum of a host-visible reduction whose producer wrote tagged word pairs: spin on pinned memory until every pair carries `tag`; nothing was put in the
    // stream for it.  NaN: a pair never arrived.
    double pollTaggedSum(const Reduction& R, unsigned tag) {
        const unsigned long long* w = reinterpret_cast<const unsigned long long*>(R.partials);
        double s = 0;
        for (int i = 0; i < R.n; ++i) {
            unsigned long long lo, hi;
            if (!spinUntil([&] {
                    lo = __atomic_load_n(w + 2 * i, __ATOMIC_ACQUIRE); hi = __atomic_load_n(w + 2 * i + 1, __ATOMIC_ACQUIRE);
                    return (unsigned)(lo >> 32) == tag && (unsigned)(hi >> 32) == tag; })) {
                fprintf(stderr, "Opt(amd): Q partial %d of tag %u never arrived (the producing launch was not issued or faulted); this early-out test is skipped and the plan goes back to reading Q through the stream\n", i, tag);
                return std::nan("");
            }
            const unsigned long long bits = (lo & 0xffffffffull) | (hi << 32);
            double v; memcpy(&v, &bits, sizeof v); s += v;
        }
        return s;
    }
    // dst[i] = sum over ranks of sum(Rs[i].partials): one launch if the communicator folds the local reduction in (allReducePartials)
    void reduceAcross(const Reduction* Rs, int cnt, double* dst) {
        if (commExt.allReducePartials) {
            const double* ps[8]; int ns[8];
            for (int i = 0; i < cnt; ++i) { ps[i] = Rs[i].partials; ns[i] = Rs[i].n; }
            commExt.allReducePartials(comm.ctx, ps, ns, cnt, dst, (void*)stream);
            return;
        }
        if (cnt == 4) {
            Partials4 in4; for (int i = 0; i < 4; ++i) { in4.p[i] = Rs[i].partials; in4.n[i] = Rs[i].n; }
            k_finalizeSum4<<<4, kBlock, 0, stream>>>(in4, dst);
        } else for (int i = 0; i < cnt; ++i) k_finalizeSum<<<1, kBlock, 0, stream>>>(Rs[i].partials, Rs[i].n, dst + i);
        comm.allReduceSum(comm.ctx, dst, cnt, (void*)stream);
    }
    // What device consumers should sum: the partials themselves, or (slab mode) the all-reduced total.
    Reduction forConsumers(const Reduction& R, int slot) {
        if (!distributed) return R;
        double* tot = scal + 3 + slot;
        reduceAcross(&R, 1, tot);
        Reduction out; out.partials = tot; out.n = 1; return out;
    }
    void finalizeTo(const Reduction& R, double* dst) {
        ScopedKernel k(ctx, "finalizeSum");
        if (distributed) reduceAcross(&R, 1, dst);
        else k_finalizeSum<<<1, kBlock, 0, stream>>>(R.partials, R.n, dst);
    }

    // ---- halo exchange (slab mode) ------------------------------------------------------------------
    void exchangeRows(const std::vector<T*>& bases) {   // one grouped exchange for all unknown images
        const Slab& s = E->slab;
        const void* su[8]; const void* sd[8]; void* ru[8]; void* rd[8]; long bytes[8];
        const int nb = (int)bases.size();
        for (int i = 0; i < nb; ++i) {
            const long rs = E->rowScalars(i % (int)E->unknowns.size()); T* base = bases[i];   // bases: one per unknown image, possibly for several vectors
            su[i] = base + (long)s.yBegin * rs; sd[i] = base + (long)(s.yEnd - s.ghost) * rs;          // my first / last `ghost` owned rows
            ru[i] = base + (long)(s.yBegin - s.ghost) * rs; rd[i] = base + (long)s.yEnd * rs; bytes[i] = (long)s.ghost * rs * (long)sizeof(T);
        }
        comm.haloExchange(comm.ctx, nb, su, sd, ru, rd, bytes, (void*)stream);
    }
    void exchangeVector(T* v) {
        if (!distributed) return;
        std::vector<T*> bases;
        for (size_t i = 0; i < E->unknowns.size(); ++i) bases.push_back(v + E->unknowns[i].offset);
        exchangeRows(bases);
    }
    void exchangeUnknowns() {
        if (!distributed) return;
        std::vector<T*> bases;
        for (size_t i = 0; i < E->unknowns.size(); ++i) bases.push_back(E->unknownPtr((int)i));
        exchangeRows(bases);
    }

    // ---- pieces ---------------------------------------------------------------------------------------
    T computeCost() {   // solver.t:790-797
        Reduction& R = distributed ? redC : redCH;   // single GPU: the partials land in pinned memory and the host sums them after one drain
        E->evalCost(R, ctx);
        return (T)hostSum(R);
    }
    void costTransition(T newCost) {      // an accepted step's cost as the reference prints it
        if (verbosity > 0) printf("cost: %f -> %f\n", (double)prevCost, (double)newCost);
        prevCost = newCost;
    }
    enum class ImageOp { update, saveAndUpdate, revert };      // X += delta (PCGLinearUpdate); prevX = X, then X += delta (LM); X = prevX (revertUpdate)
    void imageOp(ImageOp op) {
        for (size_t i = 0; i < E->unknowns.size(); ++i) {
            const auto& u = E->unknowns[i];
            long cnt = u.elems * u.channels;
            int grid = (int)std::max<long>(1, std::min<long>((cnt + kBlock - 1) / kBlock, 4096));
            T* X = E->unknownPtr((int)i);
            if (op == ImageOp::update) { ScopedKernel k(ctx, "PCGLinearUpdate"); k_axpyImage<T><<<grid, kBlock, 0, stream>>>(X, delta + u.offset, cnt); }
            else if (op == ImageOp::saveAndUpdate) { ScopedKernel k(ctx, "PCGLinearUpdate"); k_saveAndUpdate<T><<<grid, kBlock, 0, stream>>>(X, prevX + u.offset, delta + u.offset, cnt); }
            else { ScopedKernel k(ctx, "revertUpdate"); k_copy<T><<<grid, kBlock, 0, stream>>>(X, prevX + u.offset, cnt); }
        }
    }
    void record(int lIter, const Reduction& aDenR, const Reduction& bNumR, double q) {      // (bNumR in slab mode: forConsumers' all-reduced total)
        if (!traceEnabled) return;
        const double aDen = hostSum(aDenR), bNum = distributed ? readBack(bNumR.partials, 1)[0] : hostSum(bNumR), aNum = readBack(scal + aSlot, 1)[0];
        trace.insert(trace.end(), {(double)sp.nIter, (double)lIter, aNum, aDen, bNum, q});
    }

    // ---- pieces the linear-solve paths share ----------------------------------------------------------
    void initFinish() {      // PCGInit1_Finish (solver.t:384-392, 399-419): p = M r, delta = 0 and the partial sums of r.p behind evalJTF
        ScopedKernel k(ctx, "PCGInit1_Finish");
        k_initFinish<T><<<streamGrid, kBlock, 0, stream>>>(r, CtC, preconditioner, p, delta, nPacks, E->usePreconditioner ? 1 : 0, E->usesGraph ? 1 : 0, redC.partials);
        redC.n = streamGrid;
    }
    // the last PCGStep2 shrunk to delta += alpha p (+ what a launch left owed); alphaNumerator: aNum's partials, or aNumTotal if it has none
    void step2Delta(const T* pv, const double* aNumTotal, const Reduction& aNum, const Reduction& aDen, const T* pOwed = nullptr, const T* aOwed = nullptr) {
        ScopedKernel k(ctx, "PCGStep2_delta");
        k_step2FirstHalf<T><<<streamGrid, kBlock, 0, stream>>>(delta, delta, pv, nPacks, aNumTotal, aNum.partials, aNum.n, aDen.partials, aDen.n, pOwed, aOwed);
    }
    // LM's split residual reset (solver.t:1077-1083): deltaOut = delta (+ the owed term) + alpha pv with alpha as in step2Delta, then r = b - (J^T J + CtC) deltaOut
    // afresh, z = M r and the partial sums of the beta numerator (redB) and of Q (Q).  deltaOnly: r, z and the sums are dead, the reference's computeAdelta and second
    // half are not run.  fusible: the kernel set may do those two in one pass (applyJTJResetLM) -- asked on behalf of the launch-per-iteration loop only.
    void splitResidualReset(T* deltaOut, const T* pv, const T* preArg, const double* aNumTotal, const Reduction& aNum, const Reduction& aDen, Reduction& Q,
                            bool fusible, bool deltaOnly = false, const T* pOwed = nullptr, const T* aOwed = nullptr) {
        { ScopedKernel k(ctx, "PCGStep2_1stHalf");
          k_step2FirstHalf<T><<<streamGrid, kBlock, 0, stream>>>(delta, deltaOut, pv, nPacks, aNumTotal, aNum.partials, aNum.n, aDen.partials, aDen.n, pOwed, aOwed); }
        if (deltaOnly) return;
        exchangeVector(deltaOut);
        if (fusible && E->applyJTJResetLM(deltaOut, r, b, preArg, z, CtC, redB, Q, ctx)) return;
        E->applyJTJ(deltaOut, Adelta, CtC, nullptr, ctx);             // computeAdelta (+_Graph)
        { ScopedKernel k(ctx, "PCGStep2_2ndHalf");
          k_step2SecondHalf<T><<<streamGrid, kBlock, 0, stream>>>(deltaOut, r, Adelta, b, preArg, z, nPacks, redB.partials, Q.partials); }
        redB.n = streamGrid; Q.n = streamGrid;
    }
    // After the last iteration of a linear solve only delta survives: r, z, the beta numerator and -- unless someone listens for the "breaking" message or the
    // trace -- Q are dead, so the last PCGStep2, or the last split residual reset, shrinks to its delta += alpha p and LM's fetchQ (solver.t:1098) is not performed.
    bool onlyDeltaSurvives(int lIter) const { return lIter + 1 >= sp.lIterations && !traceEnabled && (!lm || verbosity == 0); }
    bool qEarlyOut(int k, T Q1, T Q0, T tol) {      // LM's q-based early out after k iterations (solver.t:1093-1102)
        const T zeta = T(k) * (Q1 - Q0) / Q1;
        if (zeta < tol && verbosity > 0) printf("zeta=%.18g, breaking at iteration: %d\n", (double)zeta, k);
        return zeta < tol;
    }
    T modelCostChange(T model_cost) {      // LM's model cost as the reference prints it (solver.t:1108-1113); returns the model cost change
        if (verbosity > 0) printf(" cost=%f \n model_cost=%f \n", (double)prevCost, (double)model_cost);
        const T change = prevCost - model_cost;
        if (verbosity > 0) printf(" model_cost_change=%f \n", (double)change);
        return change;
    }
    [[noreturn]] void refusedMidLoop() { fprintf(stderr, "pcgIteration refused mid-loop\n"); exit(1); }      // (a kernel set refused a launch after accepting the first)
    // One trace row of a single-kernel iteration from its sums alphaNumerator, alphaDenominator, s2 = sum M r.Ap, s3 = sum M Ap^2: the beta numerator by expansion,
    // sum M (r - alpha Ap)^2 = rr - 2 alpha s2 + alpha^2 s3 (clamped at 0).  quarter: an energy that does not precondition starts from p_0 = r_0 / 4 (guardedInvert(1))
    // but continues with z = r, so the first alphaNumerator is a quarter of sum r_0^2 -- which is what the expansion needs (see march_pcgIter, stencil_march.h).
    void traceRow(int k, double aNum, double aDen, double s2, double s3, bool quarter) {
        const T al = ((T)aDen > T(0)) ? (T)aNum / (T)aDen : T(0);
        const double rr = quarter ? 4.0 * aNum : aNum;
        const double bNum = std::fmax(rr - 2.0 * (double)al * s2 + (double)al * (double)al * s3, 0.0);
        trace.insert(trace.end(), {(double)sp.nIter, (double)k, aNum, aDen, bNum, 0.0});
    }

    // Row slabs: the on-chip solve runs on ALL ranks or on none (their kernels wait for each other): every rank says whether it could, the communicator adds it up.
    // (The vote comes before anything is exchanged: the launch-per-iteration loop needs r = 0 on ghost rows.)
    Solved trySlabOnChip(const T* preArg) {
        if (!allRanksAgree(onChipAllowed() && preArg && sp.lIterations > 0 && !traceEnabled && E->slabOnChipAvailable(sp.lIterations))) return {};
        (void)takeLease();      // (agreed collectively: this rank launches whether or not another plan of this process holds the chip)
        exchangeVector(r); exchangeVector(p);      // the kernel reads r_0, p_0 of its halo rows from the ghost rows
        // A rank whose kernel set refuses after the vote (it should not: the vote covers the communicator's capacity and error state) launches nothing; its
        // peers' waits then time out, and the verdict below makes every rank redo the step with the streaming loop -- a library does not exit().
        const bool refused = !E->pcgSolveOnChip(r, p, delta, sp.lIterations, nullptr, nullptr, ctx);
        if (refused) fprintf(stderr, "Opt(amd): the slab on-chip solve was agreed on but refused by this rank's kernel set; the step will be redone by the streaming loop\n");
        // all ranks keep their update or none does: the ranks' verdicts (0 fine / 1 a wait timed out) are all-reduced on the device, PCGLinearUpdate checks the sum
        E->onChipVerdict(scal + 5, refused, ctx);
        comm.allReduceSum(comm.ctx, scal + 5, 1, (void*)stream);
        E->onChipApply(delta, scal + 5, refused, ctx);
        return {Path::onChip, true};
    }
    // One GPU: the whole linear solve as one persistent launch with the loop state on chip, if the kernel set has one and the problem fits (iw_onchip.h, sfs_onchip.h,
    // stencil_onchip.h).  Gauss-Newton (lmc == nullptr): it ends with PCGLinearUpdate, guarded by the launch's failure word; a traced solve gets its per-iteration
    // scalars from the kernel.  Levenberg-Marquardt: CtC, the q early-out and the split residual reset happen on chip, the host sees only delta -- and, for a
    // listening caller (verbosity > 0), the iteration and zeta of the early-out in a pinned word, from which the reference's "breaking at iteration" message is
    // printed once the step has drained (afterLinearSolve; verbose and silent runs take the SAME path).  Not reproduced there: the message of an early-out decided
    // after the LAST iteration (its test is dead -- the loop has ended -- and the on-chip kernels do not form it).
    Solved tryOnChip(const T* preArg, const OnChipLm<T>* lmc) {
        if (!((preArg || chip) && onChipAllowed() && sp.lIterations > 0 && takeLease())) return {};
        double* tr = nullptr;
        if (traceEnabled) {
            if (onChipTraceCap < sp.lIterations) { if (onChipTrace) HIP_CHECK(hipFree(onChipTrace)); onChipTraceCap = sp.lIterations; HIP_CHECK(hipMalloc((void**)&onChipTrace, sizeof(double) * 4 * onChipTraceCap)); }
            tr = onChipTrace;
        }
        OnChipLm<T> la = lmc ? *lmc : OnChipLm<T>{};
        if (lmc) { if (!lmBreak) lmBreak = (double*)allocPinned(64); lmBreak[0] = 0.0; lmBreak[1] = 0.0; la.breakInfo = verbosity > 0 ? lmBreak : nullptr; }
        if (!E->pcgSolveOnChip(r, p, delta, sp.lIterations, tr, lmc ? &la : nullptr, ctx)) { dropLease(); return {}; }
        constexpr int kRows = 2 * kMaxPartials / 4;      // rows of four that fit hostBuf: one copy for any usual lIterations
        for (int k0 = 0; traceEnabled && k0 < sp.lIterations; k0 += kRows) {
            const int rows = std::min(kRows, sp.lIterations - k0);
            const double* h = readBack(onChipTrace + 4 * k0, 4 * rows);
            for (int k = 0; k < rows; ++k) traceRow(k0 + k, h[4 * k], h[4 * k + 1], h[4 * k + 2], h[4 * k + 3], false);
        }
        return {Path::onChip, !lmc};
    }
    // What both launch-per-iteration loops tell a launch: from (r, Ap_X, p) into the alternate buffers, the previous launch's four sums in, this launch's into setS[cur]
    PcgIterArgs<T> iterArgs(const T* preArg, bool first, const Reduction (&prev)[4], int cur, PcgIterResult<T>* result) {
        PcgIterArgs<T> a{};
        a.rOld = r; a.ApOld = Ap_X; a.pOld = p; a.rNew = r2; a.ApNew = Ap2; a.pNew = p2; a.delta = delta; a.pre = preArg; a.first = first;
        a.aNumPrev = prev[0]; a.aDenPrev = prev[1]; a.s2Prev = prev[2]; a.s3Prev = prev[3];
        a.aNum = &setS[cur][0]; a.aDen = &setS[cur][1]; a.s2 = &setS[cur][2]; a.s3 = &setS[cur][3];
        a.result = result;
        return a;
    }
    // ---- Gauss-Newton PCG loop as one kernel launch per iteration (energy.h PcgIterArgs); Path::none if the energy has no such kernel ----
    Solved runLaunchPerIterationGN(const T* preArg) {
        Reduction prev[4] = {redC, Reduction{}, Reduction{}, Reduction{}};   // alphaNum_0 = sum r.p from PCGInit1
        if (distributed) {   // ghost rows of r_0, M and p_0 (written as 0 by evalJTF / PCGInit1_Finish) come from the slab neighbours once
            exchangeVector(r); exchangeVector(p); if (preArg) exchangeVector(preconditioner);
            prev[0] = forConsumers(redC, 0);
        }
        int cur = 0;
        OptAmd_MailRef mail{nullptr, 0, 0, 0, 0, nullptr};      // where the next launch finds the previous launch's sums if they were posted, not reduced
        const IterTraits traits = E->iterTraits(false);
        for (int lIter = 0; lIter < sp.lIterations; ++lIter) {
            PcgIterResult<T> done;
            PcgIterArgs<T> a = iterArgs(preArg, lIter == 0, prev, cur, &done);
            a.mail = mail;
            // the all-reduce of THIS launch's sums, carried out by the launch itself if the communicator can plan it and the kernel set can post
            bool planned = false;
            OptAmd_MailRef nextMail{nullptr, 0, 0, 0, 0, nullptr};
            if (distributed && commExt.allReducePlan && lIter + 1 < sp.lIterations && !traceEnabled && traits.postsItself)
                planned = commExt.allReducePlan(comm.ctx, 4, &a.post, &nextMail) != 0;
            if (distributed && lIter > 0 && !traits.stateExchange) exchangeVector(Ap_X);   // kernel with Ap in memory: r and p ghost rows are kept current by the kernel itself
            deltaTrial.beforeLaunch(*this, lIter); a.delta = delta;
            if (!E->pcgIteration(a, ctx)) { if (lIter == 0) return {}; refusedMidLoop(); }
            std::swap(r, r2); std::swap(Ap_X, Ap2); std::swap(p, p2);
            if (distributed && traits.stateExchange && done.exchangeDue) {   // Ap-free kernel: the neighbours' edge rows of r_k and p_k, one grouped exchange
                std::vector<T*> bases;
                T* own[2] = {r, p};
                T* const* vecs = done.nExchange ? done.exchange : own;
                const int nv = done.nExchange ? done.nExchange : 2;
                for (int v = 0; v < nv; ++v) for (size_t i = 0; i < E->unknowns.size(); ++i) bases.push_back(vecs[v] + E->unknowns[i].offset);
                exchangeRows(bases);
            }
            for (int i = 0; i < 4; ++i) prev[i] = setS[cur][i];
            mail = OptAmd_MailRef{nullptr, 0, 0, 0, 0, nullptr};
            if (distributed) {   // one all-reduce of the four sums (ping-pong destination, like the partial sets it replaces)
                // If the communicator can POST it and the next launch's prologue can poll the mailbox, nothing waits between the two launches: the
                // contributions cross the links while the next kernel is being launched and requests its first rows.  The last iteration's sums are needed
                // by the flat kernel that closes the loop: those take the complete all-reduce.
                bool posted = planned;
                if (planned) mail = nextMail;
                if (!posted && commExt.allReducePost && traits.takesMail && lIter + 1 < sp.lIterations && !traceEnabled) {
                    const double* ps[4]; int ns[4];
                    for (int i = 0; i < 4; ++i) { ps[i] = setS[cur][i].partials; ns[i] = setS[cur][i].n; }
                    posted = commExt.allReducePost(comm.ctx, ps, ns, 4, &mail, (void*)stream) != 0;
                }
                if (!posted) {
                    double* tot = scal4[cur];
                    reduceAcross(setS[cur], 4, tot);
                    for (int i = 0; i < 4; ++i) { prev[i].partials = tot + i; prev[i].n = 1; }
                }
            }
            if (traceEnabled) {      // (four reads in this order: aNum, aDen, s2, s3 -- all-reduced already in slab mode)
                double h[4];
                for (int i = 0; i < 4; ++i) h[i] = sumOf(readBack(prev[i].partials, prev[i].n), prev[i].n);
                traceRow(lIter, h[0], h[1], h[2], h[3], lIter == 0 && !preArg && !E->usesGraph);
            }
            cur ^= 1;
        }
        // the last iteration's delta += alpha p (PCGStep2, solver.t:461-462); r, z, p of that iteration are dead.  A kernel set may fold it, its own
        // deferred terms and PCGLinearUpdate into one pass over the unknowns (EnergyOps::finishUpdate).
        if (!distributed && !traceEnabled && sp.lIterations > 0 && E->finishUpdate(delta, prev[0], prev[1], ctx)) return {Path::perIteration, true};
        const T* pLast = E->pcgFinish(delta, ctx);
        if (!pLast) pLast = p;
        finalizeLocal(prev[0], scal + 2);
        step2Delta(pLast, scal + 2, Reduction{}, prev[1]);
        return {Path::perIteration, false};
    }
    // ---- the same for Levenberg-Marquardt (energy.h PcgIterArgs, LM fields).  Launch k applies Step2 and Step3 of iteration k-1 and
    // delivers Q_{k-1}, so the q early-out of iteration k-1 (solver.t:1093-1102) is decided after launch k -- by which time the
    // state is exactly the reference's at its break (Step3 runs before fetchQ there too).  Every residual_reset_period-th iteration
    // ends with the reference's split Step2 (delta, A delta, r = b - A delta; :1077-1083) on the generic kernels; the next launch then
    // restarts from that r with beta given directly.  Path::none (nothing touched) if the energy has no such kernel.
    Solved runLaunchPerIterationLM(const T* preArg) {
        const Solved ran{Path::perIteration, false};
        T Q0 = 0;                                                   // (initLinearSystem: Q_0 is 0)
        if (!delta2) delta2 = allocVec();                       // zero-filled like delta; every launch that updates delta rewrites all of it
        Reduction prev[4] = {redC, Reduction{}, Reduction{}, Reduction{}};
        int cur = 0;
        bool afterReset = false, deltaOwed = false, issued = false, issuedRestart = false;
        Reduction bNumDirect{}, bDenDirect{};
        double qDirect = 0;                                         // Q as the last split residual reset summed it (PcgIterArgs::qInit of the restart launch)
        unsigned tagOf[2] = {0, 0};                                 // tag of the Q partials in redQ / redQ2
        PcgIterResult<T> issuedRes, adopted;                        // what the launch issued last / adopted last reported (they differ while a speculative launch is outstanding)
        auto pNow = [&]() -> const T* { return adopted.p ? adopted.p : p; };      // p of the launch adopted last (a kernel set may keep the directions in buffers of its own)
        // One launch from the current state into the alternate buffers (r2, p2, delta2, setS[cur]); adopted later by pointer swaps.
        auto issue = [&](int k, bool restart) -> bool {
            issuedRes = PcgIterResult<T>{};
            PcgIterArgs<T> a = iterArgs(preArg, k == 0, prev, cur, &issuedRes);
            a.deltaOut = delta2; a.CtC = CtC; a.b = b; a.q = (k & 1) ? &redQ2 : &redQ; a.afterReset = restart ? 1 : 0; a.betaNum = bNumDirect; a.betaDen = bDenDirect; a.qInit = qDirect;
            if (taggedQ) { if (++launchTag == 0) ++launchTag; a.qTag = tagOf[k & 1] = launchTag; } else tagOf[k & 1] = 0;      // (0: this launch writes plain partials)
            a.lmRadius = trust_region_radius; a.lmMinDiag = min_lm_diagonal; a.lmMaxDiag = max_lm_diagonal;
            issuedRestart = restart;
            return E->pcgIteration(a, ctx);
        };
        for (int lIter = 0; lIter < sp.lIterations; ++lIter) {
            if (!issued && !issue(lIter, afterReset)) { if (lIter == 0) return {}; refusedMidLoop(); }
            issued = false;
            // adopt launch lIter
            const bool appliedStep2 = lIter > 0 && !issuedRestart;    // it finished iteration lIter-1 (delta, r, z, p) and summed Q_{lIter-1}
            std::swap(r, r2); std::swap(p, p2); std::swap(Ap_X, Ap2);
            adopted = issuedRes;
            if (appliedStep2 && adopted.wroteDelta) std::swap(delta, delta2);      // (a kernel set that pairs its delta updates writes every second launch; what a deferring launch owes: adopted.owedP)
            for (int i = 0; i < 4; ++i) prev[i] = setS[cur][i];
            cur ^= 1;
            afterReset = false;
            const bool resetNow = sp.residual_reset_period > 0 && ((lIter + 1) % sp.residual_reset_period) == 0;      // (a period of 0: never -- Lua's x % 0 is nan, solver.t:1077)
            // The split residual reset (solver.t:1077-1083) of this iteration: delta += alpha p, then r = b - (J^T J + CtC) delta afresh.
            // After the last iteration of a silent solve the reference's computeAdelta and second half are not run (onlyDeltaSurvives).
            const bool deltaOnly = onlyDeltaSurvives(lIter);
            auto resetKernels = [&](T* deltaOut) {
                // (a term the adopted launch left owed goes in first, in the same pass; `delta` itself stays as it is: an early-out decided below flushes it there)
                splitResidualReset(deltaOut, pNow(), preArg, nullptr, prev[0], prev[1], redQR, true, deltaOnly, appliedStep2 ? adopted.owedP : nullptr, appliedStep2 ? adopted.owedAlpha : nullptr);
            };
            bool resetIssued = false;
            if (appliedStep2) {
                const bool tagged = tagOf[lIter & 1] != 0;      // how THIS launch wrote its Q partials (taggedQ may have been switched off since it was issued)
                if (!tagged) beginHostSum((lIter & 1) ? redQ2 : redQ);
                // What follows is enqueued before Q is known.  The next launch writes only the alternate buffers, and the reset writes delta2, r (dead after
                // an early-out) and scratch: if the test below ends the linear solve, their results are simply never adopted (the fetchQ of solver.t:1098
                // no longer idles the GPU).
                if (resetNow) { resetKernels(delta2); resetIssued = true; }
                else if (lIter + 1 < sp.lIterations) { if (!issue(lIter + 1, false)) refusedMidLoop(); issued = true; }
                const T Q1 = (T)(tagged ? pollTaggedSum((lIter & 1) ? redQ2 : redQ, tagOf[lIter & 1]) : endHostSum());
                if (Q1 != Q1) {      // a tagged Q partial never arrived (pollTaggedSum said why): this iteration's test is skipped, Q0 stays the last known value, and the
                    taggedQ = false; //  plan reads Q through the stream (beginHostSum / endHostSum) from here on, so the later early-out tests are real again
                } else {
                    if (qEarlyOut(lIter, Q1, Q0, (T)sp.q_tolerance)) { if (adopted.owedP) E->addOwedTerm(delta, adopted.owedP, adopted.owedAlpha, ctx); return ran; }
                    Q0 = Q1;
                }
            }
            deltaOwed = true;                                          // iteration lIter: Step1 done, its Step2 still to come
            if (resetNow) {
                if (resetIssued) std::swap(delta, delta2); else resetKernels(delta);
                deltaOwed = false;
                // fetchQ (solver.t:1098).  After the last iteration its only effect is the message below: the loop ends either way, so the blocking
                // read (one drain of the stream per outer iteration when residual_reset_period == lIterations, the default) happens only when someone is listening.
                if (!deltaOnly) {
                    qDirect = hostSum(redQR);
                    const T Q1 = (T)qDirect;
                    if (qEarlyOut(lIter + 1, Q1, Q0, (T)sp.q_tolerance)) return ran;
                    Q0 = Q1;
                }
                afterReset = true; bNumDirect = redB; bDenDirect = prev[0];
            }
        }
        if (deltaOwed) {   // the last iteration's delta += alpha p; its r, z, p and Q are dead (the reference's last fetchQ can only break a finished loop)
            step2Delta(pNow(), nullptr, prev[0], prev[1], adopted.owedP, adopted.owedAlpha);      // (... behind the term a deferring last launch left owed)
        }
        return ran;
    }
    void finalizeLocal(const Reduction& R, double* dst) { k_finalizeSum<<<1, kBlock, 0, stream>>>(R.partials, R.n, dst); }

    // ---- init (solver.t:956-1007) ---------------------------------------------------------------------
    void init(void** params) override {
        timer.reset(); trace.clear();
        if (overallOpen) { timer.pool.push_back(overallStart); overallOpen = false; }
        if (timer.enabled) { overallStart = timer.get(); HIP_CHECK(hipEventRecord(overallStart, stream)); overallOpen = true; }   // "overall": init -> cleanup (solver.t:959, 1011)
        tellOnChipLevel();
        E->bind(params, ctx);
        boundForSolve = insideSolve;
        sp.nIter = 0; patchSweep = 0;
        if (lm) {
            trust_region_radius = (T)sp.trust_region_radius; radius_decrease_factor = (T)sp.radius_decrease_factor;
            min_lm_diagonal = (T)sp.min_lm_diagonal; max_lm_diagonal = (T)sp.max_lm_diagonal;
        }
        exchangeUnknowns();
        E->precompute(ctx);
        // (inside Opt_ProblemSolve the first step follows at once on the same unknowns: its PCGInit1 rides on this cost pass where the kernel set can -- see initLinearSystem)
        jtfReady = false; pendingSteps.clear(); if (chip) chip->setStepSlot(-1);
        if (boundOncePerSolve() && sp.nIterations > 0 && gnInitByKernelSet() &&
            E->evalCostAndJTFInit(redCH, r, p, delta, nPad, redC, ctx)) { jtfReady = true; prevCost = (T)hostSum(redCH); }
        else prevCost = computeCost();
    }
    void cleanup() {   // solver.t:1009-1014
        if (verbosity > 0) printf("final cost=%f\n", (double)prevCost);
        if (timer.enabled) {
            if (overallOpen) { timer.closeRun(stream); KernelTimer::Rec rec{"overall", overallStart, timer.get()}; HIP_CHECK(hipEventRecord(rec.b, stream)); timer.recs.push_back(rec); overallOpen = false; }
            timer.evaluate();
            if (verbosity > 0) timer.print();
        }
    }

    // ---- step of the block-local solver (control flow of the reference comparator, PatchSolverWarping.cu:211-241) ----
    // nIterations outer steps of lIterations sweeps; sweep s shifts the patch tiling by the s-th point (mod 8) of the Halton sequence in bases
    // (2, 3), scaled by the patch size (:208-209).  Each sweep re-linearises at the current unknowns inside its kernel, so there is no global
    // r / p / delta and no grid-wide sum in the loop: one launch per sweep, the cost once per outer step.
    static double radicalInverse(int i, int base) { double f = 1, r = 0; while (i > 0) { f /= base; r += f * (i % base); i /= base; } return r; }
    int stepPatch(void** params) {
        E->bind(params, ctx);
        if (sp.nIter >= sp.nIterations) { cleanup(); return 0; }
        for (int lIter = 0; lIter < sp.lIterations; ++lIter) {
            const int o = patchSweep % 8;
            if (!E->patchIteration((float)radicalInverse(o, 2), (float)radicalInverse(o, 3), sp.patchIterations, sp.patchSize, ctx)) {
                fprintf(stderr, "patchGaussNewtonGPU: unsupported patchSize %d (16 or 32)\n", sp.patchSize); exit(1);
            }
            ++patchSweep;
        }
        E->patchFinish(ctx);
        E->precompute(ctx);
        costTransition(computeCost());
        sp.nIter += 1;
        return 1;
    }

    // ---- step (solver.t:1016-1177) --------------------------------------------------------------------
    // A step whose on-chip linear solve failed on an energy without a launch-per-iteration loop of its own is run again from its PCGInit1 on the generic kernels (the on-chip
    // path is off by then): a loop, not a recursion.
    int step(void** params) override {
        if (patch) return stepPatch(params);
        for (int attempt = 0;; ++attempt) {
            bool again = false;
            const int rc = stepOnce(params, again);
            if (!again || attempt >= 1) return rc;
        }
    }
    // Behind a drain: the costs of the deferred steps in order (printed as the reference prints them), and the first step whose on-chip solve gave up, or -1.
    int settlePending() {
        int failed = -1;
        for (const PendingStep& ps : pendingSteps) {
            if (ps.onChip && chip->stepFailed(ps.slot)) { failed = ps.step; break; }
            costTransition((T)sumOf(costRing[ps.slot].partials, costRing[ps.slot].n));
            lastStepOnChip = ps.onChip;
        }
        pendingSteps.clear();
        if (chip) chip->clearStepSlots();
        return failed;
    }
    // The deferred step `f` found its on-chip solve timed out: nothing has been applied from it on (the flag is sticky: later launches return at once and every guarded
    // update is skipped), so the solve goes back to step f on the streaming kernels.  r, p of the newest cost + PCGInit1 pass belong to exactly those unknowns.
    void rewindTo(int f) {
        (void)chip->failedNow();      // (consumes the launch's failure word)
        onChipFailure("the solve goes back to that step");
        lastStepOnChip = false;
        sp.nIter = f;
    }
    void tellOnChipLevel() { E->onChipLevel = sp.amd_onchip; E->onChipWorkgroups = sp.amd_onchip_workgroups; E->onChipPre = preconditioner; E->graphFused = sp.amd_graph_fused != 0 && sp.amd_reference_order == 0;
                             E->stencilFused = sp.amd_stencil_fused != 0 && sp.amd_reference_order == 0; }      // (EnergyOps::onChipLevel, graphFused, stencilFused)
    int stepOnce(void** params, bool& again) {
        tellOnChipLevel();
        if (!boundOncePerSolve()) E->bind(params, ctx);
        const bool mayDefer = !lm && !distributed && insideSolve && !traceEnabled && E->supportsDeferredSteps();
        if (!pendingSteps.empty() && (!mayDefer || sp.nIter >= sp.nIterations)) {      // (cannot happen: the last step of a solve is never deferred -- kept so that no cost is ever lost)
            drain();
            const int f = settlePending();
            if (f >= 0) { rewindTo(f); jtfReady = false; }
        }
        if (sp.nIter >= sp.nIterations) { cleanup(); return 0; }
        const int deferSlot = mayDefer ? (int)pendingSteps.size() : -1;
        if (chip) chip->setStepSlot(deferSlot);
        const T* preArg = E->usePreconditioner ? preconditioner : nullptr;   // solver.t:467-470: pre = 1 unless the energy preconditions
        const Init init = initLinearSystem();
        const Solved solved = solveLinear(preArg, init, false);
        AfterSolve a = afterLinearSolve(deferSlot, solved);
        if (a.deferred) {      // (the lease stays with this plan until the steps are settled)
            pendingSteps.push_back({deferSlot, sp.nIter, solved.onChip()});
            sp.nIter += 1;
            onChipCleanStep();
            return 1;
        }
        if (!settleAndRedo(preArg, deferSlot, solved, a, again)) return 1;
        if (lm && !lmDecision(a.newCost, a.modelCostChange)) return 0;
        if (!lm) costTransition(a.newCost);
        sp.nIter += 1;
        onChipCleanStep();
        return 1;
    }
    // PCGInit1 [+ _Graph + _Finish]: the energy produces r = -J^T F and raw diag(J^T J) (parked in CtC) -- or, for the Gauss-Newton single-kernel loop on one GPU,
    // r, p = M r, delta = 0 and the partial sums of r.p directly (EnergyOps::evalJTFInit), or for LM on one GPU all that PCGFinalizeDiagonal does too (evalJTFInitLM).
    // LM's fetchQ behind it (solver.t:1050) is not performed: Q_0 = 1/2 sum delta . (r + b) with the delta PCGInit1 has just zeroed is exactly 0 for every finite r.
    enum class Init { carried, jtfInit, jtfInitLM, generic };      // carried: the previous step's cost pass ran this PCGInit1 (EnergyOps::evalCostAndJTFInit)
    Init initLinearSystem() {
        aSlot = 0;
        const bool carried = jtfReady && insideSolve;      // r, p and the partial sums of r.p are already there: the previous step's cost pass wrote them from these very unknowns
        jtfReady = false;
        if (gnInitByKernelSet() && (carried || E->evalJTFInit(r, p, delta, nPad, redC, ctx)))
            return carried ? Init::carried : Init::jtfInit;
        if (lm && !distributed) {
            LmInitArgs<T> la{CtC, SSq, r, delta, preconditioner, b, p, trust_region_radius, min_lm_diagonal, max_lm_diagonal, sp.nIter == 0 ? 1 : 0, &redC, &redQ};
            if (E->evalJTFInitLM(la, ctx)) return Init::jtfInitLM;
        }
        E->evalJTF(r, CtC, ctx);
        if (!lm) { initFinish(); return Init::generic; }
        ScopedKernel k(ctx, "PCGFinalizeDiagonal");      // PCGInit1_Finish + (first outer iteration) PCGSaveSSq + PCGFinalizeDiagonal in one pass
        k_finalizeDiagonal<T, true><<<streamGrid, kBlock, 0, stream>>>(CtC, SSq, r, delta, preconditioner, b, p, nPacks, trust_region_radius, min_lm_diagonal,
                                                                       max_lm_diagonal, redC.partials, redQ.partials, E->usePreconditioner ? 1 : 0,
                                                                       E->usesGraph ? 1 : 0, sp.nIter == 0 ? 1 : 0);
        redC.n = streamGrid; redQ.n = streamGrid;
        return Init::generic;
    }
    // The Levenberg-Marquardt controls an on-chip solve is asked with: solveLinear and describe pass the same, so that describe answers for the step
    OnChipLm<T> lmControls() const { return OnChipLm<T>{trust_region_radius, min_lm_diagonal, max_lm_diagonal, (T)sp.q_tolerance, sp.residual_reset_period, CtC, sp.amd_onchip}; }
    // The one place that picks the linear solve's path, the first that takes it: (1) on chip -- in slab mode behind the vote every rank issues --, (2) the kernel set's
    // launch-per-iteration loop, (3) the reference-order loop.  (1) and (2) need singleKernelAllowed() (off with OPT_AMD_ONEKERNEL=0 or amd_reference_order=1), in LM
    // also OPT_AMD_ONEKERNEL_LM, one GPU and no trace.  A redo after an on-chip time-out stops short of (3): Path::none, and the step runs again from its PCGInit1.
    Solved solveLinear(const T* preArg, Init init, bool redo) {
        if (singleKernelAllowed()) {
            Solved s;
            if (lm) {
                const OnChipLm<T> la = lmControls();
                if (oneKernelLM && !distributed && !traceEnabled && ((s = tryOnChip(preArg, &la)) || (s = runLaunchPerIterationLM(preArg)))) return s;
            } else {
                if ((s = distributed ? trySlabOnChip(preArg) : tryOnChip(preArg, nullptr))) return s;
                if ((!distributed || E->iterTraits(false).slabAvailable) && (s = runLaunchPerIterationGN(preArg))) return s;
            }
        }
        if (redo) return {};
        if (init == Init::carried || init == Init::jtfInit) {      // the kernel set accepted evalJTFInit but refused the loop (it should not): PCGInit1 again -- a library does not exit()
            fprintf(stderr, "Opt(amd): the kernel set accepted evalJTFInit but refused the single-kernel loop; this step runs on the generic kernels\n");
            E->evalJTF(r, CtC, ctx);
            initFinish();
        }
        runReferenceOrderLoop(preArg);
        return {Path::referenceOrder, false};
    }
    // The reference's loop: PCGStep1, PCGStep2, PCGStep3 per iteration (solver.t:1056-1103).  Step3 of iteration k is fused into Step1 of iteration k+1 when the energy
    // offers that kernel (it only feeds the next Step1; after the last iteration p is dead).  None of Step3 + Step1 touches what survives a q early-out (delta, and p only
    // through the very Step3 the reference also runs before its q test), so in LM it is enqueued BEFORE the host reads q of the current iteration: the blocking fetchQ of
    // solver.t:1098 then overlaps with useful kernels instead of draining the GPU once per PCG iteration.  With tracing on, the original order (decide, then launch) is kept.
    void runReferenceOrderLoop(const T* preArg) {
        finalizeTo(redC, scal + aSlot);   // alphaNumerator = sum r.p as one device scalar (the single-kernel loops sum the partials in their first launch)
        const bool speculate = !traceEnabled;
        T Q0 = 0;                         // (initLinearSystem: Q_0 is 0)
        Reduction aDen, bNum;
        if (sp.lIterations > 0) aDen = stepThreeAndOne(nullptr);     // Step1 of iteration 0
        for (int lIter = 0; lIter < sp.lIterations; ++lIter) {
            const bool reset = lm && sp.residual_reset_period > 0 && ((lIter + 1) % sp.residual_reset_period) == 0;
            if (onlyDeltaSurvives(lIter)) { step2Delta(p, scal + aSlot, Reduction{}, aDen); break; }
            if (reset) splitResidualReset(delta, p, preArg, scal + aSlot, Reduction{}, aDen, redQ, false);
            else {
                ScopedKernel k(ctx, "PCGStep2");
                if (lm) k_step2<T, true><<<streamGrid, kBlock, 0, stream>>>(delta, p, r, Ap_X, preArg, b, z, nPacks, scal + aSlot, aDen.partials, aDen.n, redB.partials, redQ.partials);
                else k_step2<T, false><<<streamGrid, kBlock, 0, stream>>>(delta, p, r, Ap_X, preArg, nullptr, z, nPacks, scal + aSlot, aDen.partials, aDen.n, redB.partials, nullptr);
                redB.n = streamGrid; redQ.n = streamGrid;
            }
            bNum = forConsumers(redB, 1);      // (PCGStep3 of this iteration runs with the next PCGStep1)
            const bool more = lIter + 1 < sp.lIterations;
            double qh = 0;
            if (lm && speculate) {
                beginHostSum(redQ);
                if (more) aDen = stepThreeAndOne(&bNum);
                qh = endHostSum();
            } else {
                if (lm) qh = hostSum(redQ);
                if (traceEnabled) record(lIter, aDen, bNum, qh);
            }
            if (lm) {   // solver.t:1093-1102
                const T Q1 = (T)qh;
                if (qEarlyOut(lIter + 1, Q1, Q0, (T)sp.q_tolerance)) break;
                Q0 = Q1;
            }
            if (more && !(lm && speculate)) aDen = stepThreeAndOne(&bNum);
        }
    }
    // PCGStep3 of the previous iteration (bNum: its beta numerator; nullptr before iteration 0) and PCGStep1 of the next one, as one kernel where the energy fuses them.
    // Returns the alpha denominator as its consumers read it.
    Reduction stepThreeAndOne(const Reduction* bNum) {
        bool applied = false;
        if (bNum) {
            exchangeVector(z);      // (an energy without the fused kernel refuses: the generic PCGStep3 below)
            applied = E->applyJTJFused(p, z, p2, Ap_X, lm ? CtC : nullptr, &redA, *bNum, scal + aSlot, scal + (aSlot ^ 1), ctx);
            if (applied) std::swap(p, p2);
            else { ScopedKernel k(ctx, "PCGStep3"); k_step3<T><<<streamGrid, kBlock, 0, stream>>>(z, p, nPacks, bNum->partials, bNum->n, scal + aSlot, scal + (aSlot ^ 1)); }
            aSlot ^= 1;   // alphaNumerator <- betaNumerator (solver.t:1091)
        }
        if (!applied) {
            exchangeVector(p);
            E->applyJTJ(p, Ap_X, lm ? CtC : nullptr, &redA, ctx);    // PCGStep1 (+_Graph)
        }
        return forConsumers(redA, 0);
    }
    // What follows the linear solve (solver.t:1108-1117): model cost, savePreviousUnknowns + PCGLinearUpdate, precompute, the new cost.  The reference reads the
    // model cost, then updates, then reads the new cost (two blocking copies); neither value steers anything before both are known, so all of it is enqueued
    // and the stream is drained once.  deferred: nothing was read back (deferSlot: this step's cost buffer, or -1).
    struct AfterSolve { T newCost = 0, modelCostChange = 0; bool deferred = false; };
    AfterSolve afterLinearSolve(int deferSlot, Solved solved) {
        AfterSolve a;
        if (lm) {   // solver.t:1108-1113, 819-827
            exchangeVector(delta);
            E->evalModelCost(delta, distributed ? redA : redMH, ctx);   // (its own partials buffer: the value is read together with the new cost below)
            imageOp(ImageOp::saveAndUpdate);
        } else if (!solved.updated) imageOp(ImageOp::update);
        exchangeUnknowns();
        E->precompute(ctx);
        if (lm && !distributed) {
            E->evalCost(redCH, ctx);                   // both sets of partials are written straight to pinned memory: one drain, no copy kernels
            drain();
            if (solved.onChip() && verbosity > 0 && lmBreak && lmBreak[0] > 0.0 && !chip->failedPeek()) { printf("zeta=%.18g, breaking at iteration: %d\n", lmBreak[1], (int)lmBreak[0] - 1); lmBreak[0] = 0.0; }
            a.newCost = (T)sumOf(redCH.partials, redCH.n);
            a.modelCostChange = modelCostChange((T)sumOf(redMH.partials, redMH.n));
            return a;
        }
        if (lm) a.modelCostChange = modelCostChange((T)hostSum(redA));
        // Gauss-Newton inside Opt_ProblemSolve with another step to come: that step's PCGInit1 reads the unknowns this cost reads, and no caller code runs in
        // between -- one pass does both where the kernel set can (same cost bits: same grid, same expressions).  A step on the generic kernels (back-off after
        // an on-chip time-out included) does not ask.
        const bool carry = boundOncePerSolve() && sp.nIter + 1 < sp.nIterations && gnInitByKernelSet();
        Reduction& costR = deferSlot >= 0 ? costRing[deferSlot] : redCH;
        if (deferSlot >= 0 && !costR.partials) { costR.partials = (double*)allocPinned(2 * kMaxPartials * sizeof(double)); costR.hostVisible = true; }
        if (carry && E->evalCostAndJTFInit(costR, r, p, delta, nPad, redC, ctx)) {
            jtfReady = true;
            if (deferSlot >= 0 && deferSlot + 1 < kDefer) a.deferred = true;      // nothing is read back now: the next step is enqueued behind this one
            else a.newCost = (T)hostSum(costR);
        } else a.newCost = computeCost();
        return a;
    }
    // Behind the cost read: the deferred steps, then this step's on-chip verdict (a time-out redoes the linear solve).  false: the step ends here.
    bool settleAndRedo(const T* preArg, int deferSlot, Solved solved, AfterSolve& a, bool& again) {
        if (!pendingSteps.empty()) {      // the stream has drained (this step's cost was read): what the deferred steps before it left
            const int f = settlePending();
            if (f >= 0) {
                // from step f on nothing was applied -- unless THIS step ran on the streaming kernels (it cannot while the path is armed; if it did, it was a valid step from
                // the unknowns of step f and counts as that step)
                rewindTo(f);
                if (!solved.onChip()) { costTransition(a.newCost); sp.nIter = f + 1; }
                return false;      // (jtfReady says whether this step's cost pass carried a PCGInit1 for the unknowns as they stand; the last step of a solve carries none)
            }
            if (!solved.onChip()) dropLease();
        }
        const bool timedOut = solved.onChip() && chip->failedNow();      // (the stream has drained: the cost was read)
        lastStepOnChip = solved.onChip() && !timedOut;
        if (!timedOut) { if (solved.onChip()) dropLease(); return true; }      // the launch has left the chip
        onChipFailure("this linear solve is redone");
        if (lm) {      // the kernel produced no delta: the update above added nothing meaningful -- back to the saved unknowns, then the launch-per-iteration loop
            imageOp(ImageOp::revert);
            E->precompute(ctx);      // (workgroups that had finished before the others gave up may have written their delta: the update above was then not the identity)
        }
        // Gauss-Newton: nothing was applied (iw_applyDelta checks the flag -- in slab mode the all-reduced verdict, so no rank kept its update).
        // The redone loop starts from delta = 0 as PCGInit1 left it: the ROWS = 16 variant accumulates delta in memory while it runs.
        HIP_CHECK(hipMemsetAsync(delta, 0, nPad * sizeof(T), stream));
        const Solved redone = solveLinear(preArg, Init::generic, true);
        if (!redone) { again = true; return false; }      // (no launch-per-iteration loop: the whole step again on the generic kernels)
        a = afterLinearSolve(deferSlot, redone);
        return true;
    }
    // LM's accept / reject (solver.t:1119-1157).  false: a tolerance was reached and the solve has ended (cleanup has run).
    bool lmDecision(T newCost, T model_cost_change) {
        const T min_relative_decrease = (T)sp.min_relative_decrease, min_trust_region_radius = (T)sp.min_trust_region_radius;
        const T max_trust_region_radius = (T)sp.max_trust_region_radius, function_tolerance = (T)sp.function_tolerance;
        T cost_change = prevCost - newCost;
        T relative_decrease = cost_change / model_cost_change;
        if (cost_change >= 0 && relative_decrease > min_relative_decrease) {
            T absolute_function_tolerance = prevCost * function_tolerance;
            if (cost_change <= absolute_function_tolerance) {
                if (verbosity > 0) printf("\nFunction tolerance reached, exiting\n");
                cleanup(); return false;
            }
            // Terra promotes these literals to double; results are stored back as opt_float (solver.t:1135-1139)
            double step_quality = (double)relative_decrease, min_factor = 1.0 / 3.0;
            double tmp_factor = 1.0 - std::pow(2.0 * step_quality - 1.0, 3.0);
            trust_region_radius = (T)((double)trust_region_radius / std::fmax(min_factor, tmp_factor));
            trust_region_radius = std::fmin(trust_region_radius, max_trust_region_radius);
            radius_decrease_factor = T(2.0);
            prevCost = newCost;
        } else {
            imageOp(ImageOp::revert);
            trust_region_radius = trust_region_radius / radius_decrease_factor;
            if (verbosity > 0) printf(" trust_region_radius=%f \n", (double)trust_region_radius);
            radius_decrease_factor = T(2.0) * radius_decrease_factor;
            if (trust_region_radius <= min_trust_region_radius) {
                if (verbosity > 0) printf("\nTrust_region_radius is less than the min, exiting\n");
                cleanup(); return false;
            }
            if (verbosity > 0) printf("REVERT\n");
            exchangeUnknowns();
            E->precompute(ctx);
            HIP_CHECK(hipStreamSynchronize(stream));   // results visible when the call returns
        }
        return true;
    }

    double cost() const override { return (double)prevCost; }   // solver.t:1179-1182
    void setTiming(int mode) override {      // per-kernel hipEvents from the next launch on (what collectPerKernelTimingInfo sets at plan time); 2: one pair per run of equal names
        HIP_CHECK(hipStreamSynchronize(stream));
        if (overallOpen) { timer.pool.push_back(overallStart); overallOpen = false; }
        const bool on = mode != 0;
        timer.reset(); timer.enabled = on; timer.coarse = mode == 2; ctx.timer = on ? &timer : nullptr;
    }
    long numUnknownScalars() const override { return n; }
    double trustRegionRadius() const override { return (double)trust_region_radius; }
    int onChipStatus() const override { return onChipOff() ? 2 : lastStepOnChip ? 1 : 0; }
    std::string describe() override {
        tellOnChipLevel();
        std::string d = sp.amd_reference_order ? std::string("path=reference-order (PCGStep1 [+ the previous PCGStep3] and PCGStep2 per PCG iteration, r / z / A p in memory); amd_reference_order=1")
                                               : [&] { const OnChipLm<T> la = lmControls(); return E->describe(sp.lIterations, lm, lm ? &la : nullptr); }();
        if (sp.amd_reference_order && sp.amd_stencil_fused) d += "; why_not_fused=amd_reference_order wins over amd_stencil_fused";
        if (!sp.amd_reference_order && sp.amd_onchip != 1) d += "; amd_onchip=" + std::to_string(sp.amd_onchip);
        if (!sp.amd_reference_order && !oneKernel) d += "; OPT_AMD_ONEKERNEL=0 (reference-order loop by environment)";
        if (onChipFailures) d += "; onchip_fallbacks=" + std::to_string(onChipFailures) + "; onchip_backoff_steps_left=" + std::to_string(onChipOff() ? onChipBackoff - onChipCleanSteps : 0);
        // what Opt_ProblemSolve does beyond Init + Step by Step on this plan, and where the trial over delta's placement stands
        if (!lm && !distributed && E->supportsDeferredSteps()) d += "; solve_enqueues_steps_back_to_back=up to " + std::to_string(kDefer - 1);
        d += deltaTrial.describe(*this);
        d += std::string("; solver=") + (lm ? "LM" : "GN") + "; distributed=" + (distributed ? "yes" : "no") + "; comm_world=" + std::to_string(distributed ? comm.world : 1) +
             "; comm_ext=" + (commExt.onChipPlan ? "onChipPlan " : "") + (commExt.allReducePost ? "allReducePost " : "") + (commExt.allReducePartials ? "allReducePartials" : "");
        return d;
    }
    void* vector(const std::string& nm) override {
        if (nm == "delta") return delta; if (nm == "r") return r; if (nm == "b") return b; if (nm == "Adelta") return Adelta;
        if (nm == "z") return z; if (nm == "p") return p; if (nm == "Ap_X") return Ap_X; if (nm == "CtC") return CtC;
        if (nm == "preconditioner") return preconditioner; if (nm == "SSq") return SSq; if (nm == "prevX") return prevX;
        return nullptr;
    }

    // ---- kernel-level probes (OptAmd.h) ---------------------------------------------------------------
    void evalJTF(void** params, void* jtf, void* diag) override {
        E->bind(params, ctx); exchangeUnknowns(); E->precompute(ctx);
        E->evalJTF(z, Ap_X, ctx);   // scratch use of z / Ap_X: z = -J^T F
        HIP_CHECK(hipStreamSynchronize(stream));
        std::vector<T> h(n);
        HIP_CHECK(hipMemcpy(h.data(), z, n * sizeof(T), hipMemcpyDeviceToHost));
        for (auto& x : h) x = -x;
        HIP_CHECK(hipMemcpy(jtf, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(diag, Ap_X, n * sizeof(T), hipMemcpyDeviceToDevice));
    }
    double applyJTJ(void** params, const void* v, void* out) override {
        tellOnChipLevel();      // (amd_graph_fused decides which kernels a functor mesh energy applies J^T J with)
        E->bind(params, ctx); exchangeUnknowns(); E->precompute(ctx);
        E->evalJTF(z, CtC, ctx);   // refreshes the energy's per-iteration auxiliaries (e.g. cos/sin tables)
        HIP_CHECK(hipMemsetAsync(p, 0, nPad * sizeof(T), stream));
        HIP_CHECK(hipMemcpyAsync(p, v, n * sizeof(T), hipMemcpyDeviceToDevice, stream));
        exchangeVector(p);
        E->applyJTJ(p, Ap_X, nullptr, &redA, ctx);
        double d = hostSum(redA);
        HIP_CHECK(hipMemcpy(out, Ap_X, n * sizeof(T), hipMemcpyDeviceToDevice));
        return d;
    }
    double evalCost(void** params) override {
        E->bind(params, ctx); exchangeUnknowns(); E->precompute(ctx);
        return (double)computeCost();
    }
    int setSlab(long row0, long rows, long globalHeight, const OptAmd_SlabComm* c) override {
        if (!E->supportsSlab() || !c || patch) return 0;   // the block-local solver is single-GPU
        // local height = rows + 2 * ghost: the plan was created with dims {W, rows + 2 * ghost}
        const long localH = E->unknowns[0].elems * E->unknowns[0].channels / E->rowScalars(0);
        const long g = (localH - rows) / 2;
        if (g < 1 || rows + 2 * g != localH) return 0;
        E->slab.active = true; E->slab.ghost = (int)g; E->slab.yBegin = (int)g; E->slab.yEnd = (int)(rows + g); E->slab.gy0 = (int)(row0 - g); E->slab.Hg = (int)globalHeight;
        comm = *c; commExt = OptAmd_SlabCommExt{};
        distributed = c->world > 1 || getenv("OPT_AMD_FORCE_COMM") != nullptr;   // the env switch lets a 1-rank test drive the comm callbacks
        return 1;
    }
    int setSlabExt(const OptAmd_SlabCommExt* e) override {      // only the members the caller's struct actually has are read
        if (!e || !E->slab.active) return 0;
        commExt = OptAmd_SlabCommExt{};
        const size_t have = (size_t)e->size;
        auto has = [&](size_t off, size_t sz) { return have >= off + sz; };
        if (has(offsetof(OptAmd_SlabCommExt, allReducePartials), sizeof(e->allReducePartials))) commExt.allReducePartials = e->allReducePartials;
        if (has(offsetof(OptAmd_SlabCommExt, allReducePost), sizeof(e->allReducePost))) commExt.allReducePost = e->allReducePost;
        if (has(offsetof(OptAmd_SlabCommExt, allReducePlan), sizeof(e->allReducePlan))) commExt.allReducePlan = e->allReducePlan;
        if (has(offsetof(OptAmd_SlabCommExt, onChipPlan), sizeof(e->onChipPlan))) { commExt.onChipPlan = e->onChipPlan; E->onChipPlan = e->onChipPlan; E->onChipCtx = comm.ctx; }
        commExt.size = sizeof(OptAmd_SlabCommExt);
        return 1;
    }
};

bool SolverBase::setParameter(const char* name, const void* value) {   // solver.t:1205-1221
    std::string nm(name);
#define PF(x) if (nm == #x) { sp.x = *(const float*)value; return true; }
#define PI(x) if (nm == #x) { sp.x = *(const int*)value; return true; }
    PF(min_relative_decrease) PF(min_trust_region_radius) PF(max_trust_region_radius) PF(q_tolerance) PF(function_tolerance)
    PF(trust_region_radius) PF(radius_decrease_factor) PF(min_lm_diagonal) PF(max_lm_diagonal)
    PI(residual_reset_period) PI(nIter) PI(nIterations) PI(lIterations) PI(patchIterations) PI(patchSize)
    PI(amd_reference_order) PI(amd_onchip) PI(amd_onchip_workgroups) PI(amd_graph_fused) PI(amd_stencil_fused)
#undef PF
#undef PI
    return false;
}

template <class T>
static SolverBase* makeSolverOf(EnergyOps<T>* e, bool lm, bool patch, bool timing, int verbosity) {
    if (!e) return nullptr;
    if (patch && !e->supportsPatch()) { delete e; return nullptr; }
    auto* s = new PcgSolver<T>(e, lm, timing, verbosity); s->patch = patch; return s;
}
SolverBase* makeSolver(const EnergyInfo& info, bool lm, bool patch, bool doublePrecision, const unsigned* dims, bool timing, int verbosity) {
    if (doublePrecision && !info.floatOnly) return makeSolverOf(info.makeDouble(dims), lm, patch, timing, verbosity);
    return makeSolverOf(info.makeFloat(dims), lm, patch, timing, verbosity);
}

}  // namespace optamd
