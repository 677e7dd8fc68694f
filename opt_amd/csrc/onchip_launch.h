// Host side of the wave-tiled on-chip linear solves -- stencil_onchip.h (5-point stencils, a one-pixel ring) and sfs_onchip.h (shape_from_shading, a two-pixel ring): the
// time-out guard, the two tagged buffers, which variant (if any) a plan takes, the protocol's kernel arguments (OcArgs, filled by OcGrant::args), the launch,
// the guarded X += delta behind a Gauss-Newton solve and describe()'s text.
// The device kernels differ; what differs for the host is data (OcFamily, the variant list).  image_warping's on-chip solve (tiles, dynamic LDS, row slabs) has a
// host side of its own (energy_image_warping.hip).
#pragma once
#include "energy.h"
#include "onchip_sync.h"

namespace optamd {
namespace {

// rows a wave owns, waves per workgroup, the kernel of each mode (nullptr: not offered): Gauss-Newton, Levenberg-Marquardt, Levenberg-Marquardt with the split residual reset inside the solve
struct OcVariant {
    int rows, waves; const void *gn, *lm, *lmReset = nullptr;
    const void* kernel(int mode) const { return mode == 0 ? gn : mode == 1 ? lm : lmReset; }
};
struct OcFamily {
    int span, halo, maxG, words;             // pixels a wave owns per row; rows it holds around its own (the cost model); workgroup cap; tagged words per workgroup
    const char *kernel, *loopGN, *loopLM;    // describe(): the kernel, the launch-per-iteration loops it stands in for
    const char* launchFailed;                // stderr text (rows, waves) when the launch itself is refused, or nullptr: silent
    int resetFrom = 2;                       // the amd_onchip value from which the family keeps a residual reset inside the solve on chip (5-point stencils: 2, shape_from_shading: 3)
};
struct OcPlan {
    const OcVariant* V = nullptr; int stripsX = 0, tilesY = 0, G = 0;
    int mode = 0, phases = 0;      // the variant's kernel (OcVariant::kernel); grid-wide waits of the solve: one per iteration and one more per in-solve residual reset (mode 2)
    explicit operator bool() const { return V != nullptr; }
};
// The kernel arguments of the protocol (onchip_sync.h ocGridSum and what goes with it): embedded in the family's own argument struct (MoArgs), filled by OcGrant::args and nowhere else.
// (SfsOcArgs keeps its own fields in its own order: its kernels' code depends on the layout, sfs_onchip.h.)
template <class T>
struct OcArgs {
    int stripsX, tilesY, G, L;
    unsigned tag0;                      // tag of iteration 0 (tags never repeat over the life of the buffers)
    oc_u64* slots;                      // [2][G][2 x sums per phase]
    oc_u64* apBox;                      // [2][W * H * C * sizeof(T) / 4]
    int* bad; long long timeoutTicks;
    long long firstTicks;               // bound of the FIRST iteration's wait: the co-residency check (every workgroup has posted its words once it passes), before anything is written
    int failAt;
    int* hostErr;                       // LM (the solver applies the update itself): pinned host word a workgroup that gave up raises on its way out; GN: nullptr (ocApplyDelta tells the host)
    const T* CtC; T qTolerance;         // LM: the clamped diagonal, q_tolerance
    double* lmBreak;                    // pinned {iteration + 1, zeta} of the q early-out (OnChipLm::breakInfo), or nullptr
    int resetPeriod;                    // MODE 2: every resetPeriod-th iteration (but the last) ends with the split residual reset
};
// What a launch is granted; the family adds its own arguments to args() and calls launch(), the launch of the chosen variant.
struct OcGrant : OcPlan {
    const void* fn; unsigned tag0; oc_u64 *slots, *box; int* bad; OcTimeouts tmo; int failAt;
    int* hostErr;      // LM (the solver applies the update itself): the pinned word a workgroup that gave up raises on its way out; Gauss-Newton: nullptr (ocApplyDelta tells the host)
    template <class T> OcArgs<T> args(int L, const OnChipLm<T>* lm) const {
        OcArgs<T> a{};
        a.stripsX = stripsX; a.tilesY = tilesY; a.G = G; a.L = L; a.tag0 = tag0; a.slots = slots; a.apBox = box;
        a.bad = bad; a.timeoutTicks = tmo.later; a.firstTicks = tmo.first; a.failAt = failAt; a.hostErr = hostErr;
        if (lm) { a.CtC = lm->CtC; a.qTolerance = lm->qTolerance; a.lmBreak = lm->breakInfo; a.resetPeriod = lm->resetPeriod; }
        return a;
    }
    bool launch(void** kargs, hipStream_t s) const { return hipLaunchKernel(fn, dim3(G), dim3(V->waves * kWave), kargs, 0, s) == hipSuccess; }
};

template <class T>
struct OnchipLauncher {
    OnchipGuard guard;      // the switches (OPT_AMD_ONCHIP*) and the time-out verdict
    oc_u64 *slots = nullptr, *box = nullptr;      // the tagged buffers: [2][maxG][words] sums, [2][W * H * C * sizeof(T) / 4] ring
    OcFamily fam{};
    const std::vector<OcVariant>& (*variants)() = nullptr;
    int W = 0, H = 0, C = 1, cus = 0;      // the plan's image (the dimensions of a plan are fixed), scalars per pixel
    long updateCap = 0;                    // workgroups of the guarded update, per unknown image
    void init(const OcFamily& f, const std::vector<OcVariant>& (*v)(), int W_, int H_, int C_, int cus_, long updateCap_) { fam = f; variants = v; W = W_; H = H_; C = C_; cus = cus_; updateCap = updateCap_; }
    // among the variants whose workgroups fit one per CU: the least marching time per SIMD and iteration
    OcPlan select(int mode) const {
        OcPlan best; int bestCost = 1 << 30;
        const int stripsX = divUp(W, fam.span);
        for (const auto& v : variants()) {
            if (!v.kernel(mode)) continue;
            if (guard.forceRows && v.rows != guard.forceRows) continue;
            if (guard.forceWaves && v.waves != guard.forceWaves) continue;
            const int ty = divUp(H, v.rows), g = divUp(stripsX * ty, v.waves);
            if (g > std::min(cus, fam.maxG)) continue;
            const int cost = (v.waves == 4 ? 100 : 136) * (v.rows + fam.halo);      // (measured: two waves per SIMD march a pair of trips in 1.36 of the time one wave marches one)
            if (cost < bestCost) { best = OcPlan{&v, stripsX, ty, g, mode, 0}; bestCost = cost; }
        }
        return best;
    }
    // THE predicate: would a linear solve of L iterations run on chip, and with which variant?  lmv: the Levenberg-Marquardt loop (lm: its controls, where the caller has
    // them).  A split residual reset before the last iteration (residual_reset_period < L) takes the family's mode-2 kernel, for a caller who opted in (amd_onchip >= OcFamily::resetFrom)
    // and where such a variant fits; otherwise it is the launch-per-iteration loop's business.  solve(), describe(), reserve() and a kernel set that wants to know before
    // it spends a coefficient pass all ask here.
    bool resetInside(int L, const OnChipLm<T>* lm) const { return lm && lm->resetPeriod < L; }
    bool offersReset() const { for (const auto& v : variants()) if (v.lmReset) return true; return false; }
    OcPlan plan(int L, bool lmv, const OnChipLm<T>* lm = nullptr) const {
        if (!guard.usable() || L <= 0 || (unsigned long long)W * H * C * sizeof(T) >= (1ull << 30)) return {};
        if (lm && !lm->CtC) return {};
        if (!resetInside(L, lm)) { OcPlan P = select(lmv ? 1 : 0); P.phases = L; return P; }
        if (lm->onchip < fam.resetFrom || lm->resetPeriod <= 0) return {};
        OcPlan P = select(2);
        P.phases = L + (L - 1) / lm->resetPeriod;
        return P;
    }
    // The buffers of the path, when the plan is made (so that its first linear solve does not pay for the allocations) -- only for plans that can take the path at all:
    // some variant fits this device's CUs for the image (a 4-channel double image of 1-2 M pixels would otherwise hold ~256 MB of tagged box it could never use)
    void reserve() {
        if (slots || !(plan(1, false) || plan(1, true))) return;
        slots = guard.allocTagged<oc_u64>(sizeof(oc_u64) * 2 * (size_t)fam.maxG * fam.words);
        box = guard.allocTagged<oc_u64>(sizeof(oc_u64) * 2 * (size_t)W * H * C * (sizeof(T) / 4));
        guard.allocWords(nullptr); guard.clearTagged(nullptr); HIP_CHECK(hipStreamSynchronize(nullptr));      // (done before the plan's own stream sees the buffers)
    }
    // The whole linear solve and, behind a Gauss-Newton one, X += delta over the kernel set's unknown images; false (nothing touched): not offered for this plan.
    // launchWith(grant): the family fills its kernel's arguments and calls grant.launch (false: the launch was refused -- the path is switched off).
    template <class Fill>
    bool solve(int L, const OnChipLm<T>* lm, const T* delta, const EnergyOps<T>& ops, LaunchCtx& ctx, Fill&& launchWith) {
        const OcPlan P = plan(L, lm != nullptr, lm);
        if (!P) return false;
        if (!slots) { reserve(); if (!slots) return false; }
        OcGrant g{P, P.V->kernel(P.mode), guard.tags((unsigned)P.phases, ctx.stream), slots, box, guard.bad, guard.timeouts(P.phases, false), guard.failAtThisLaunch(), lm ? guard.hostErr : nullptr};
        {
            ScopedKernel k(ctx, "PCGSolveOnChip");
            if (!launchWith(g)) {      // (a device that cannot hold the variant's LDS: not offered again)
                (void)hipGetLastError(); guard.enabled = false;
                if (fam.launchFailed) fprintf(stderr, fam.launchFailed, P.V->rows, P.V->waves);
                return false;
            }
        }
        if (!lm) ocApplyDeltaToUnknowns(ops, delta, updateCap, guard, ctx);      // (LM: the solver applies the update itself)
        guard.launched = true;
        return true;
    }
    // ("key=value; ..." -- no ';' inside a value)  blocked: the kernel set's own reason to keep the plan off the chip, or nullptr
    // lm: the Levenberg-Marquardt controls the plan's next step would pass to solve() -- the answer is the step's
    std::string describe(int L, bool lmv, const OnChipLm<T>* lm, const char* blocked = nullptr) const {
        const OcPlan P = blocked ? OcPlan{} : plan(L, lmv, lm);
        const bool reset = resetInside(L, lm);
        char buf[700], optIn[160];
        snprintf(optIn, sizeof optIn, "a residual reset falls inside the solve (lIterations > residual_reset_period) and amd_onchip=%d was not set", fam.resetFrom);
        if (P) snprintf(buf, sizeof buf, "path=on-chip (%s%s); onchip_rows_per_wave=%d; waves_per_workgroup=%d; wave_tiles=%dx%d of %d x %d pixels; workgroups=%d of %d CUs; fallback=one launch per PCG iteration (%s)",
                        fam.kernel, !lmv ? "" : P.mode == 2 ? ", LM with the residual resets inside the solve" : ", LM, no residual reset inside the solve", P.V->rows, P.V->waves, P.stripsX, P.tilesY, fam.span,
                        P.V->rows, P.G, cus, lmv ? fam.loopLM : fam.loopGN);
        else snprintf(buf, sizeof buf, "path=one launch per PCG iteration (%s%s); why_not_on_chip=%s", lmv ? fam.loopLM : fam.loopGN, lmv ? ", LM" : "",
                      guard.whyOff() ? guard.whyOff() : blocked ? blocked : lm && !lm->CtC ? "no LM diagonal"
                      : !reset || !select(1) ? "the wave tiles do not fit the CUs"
                      : !offersReset() ? "a residual reset falls inside the solve (lIterations > residual_reset_period) and this kernel family has no on-chip reset"
                      : lm->resetPeriod <= 0 ? "residual_reset_period <= 0"
                      : lm->onchip < fam.resetFrom ? optIn
                      : "a residual reset falls inside the solve and no variant with the reset on chip fits the CUs");
        return buf;
    }
};

}  // namespace
}  // namespace optamd
