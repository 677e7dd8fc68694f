// 5-point stencils with C channels per pixel (the operators of stencil_march.h: poisson_image_editing, the minimal laplacian, optical_flow, intrinsic_image_decomposition): the WHOLE PCG linear solve
// of a Gauss-Newton step as one persistent launch whose loop state never leaves the chip.
//
// What it replaces: the reference's loop `for lIter = 0, lIterations do PCGStep1; PCGStep2; PCGStep3 end` (solverGPUGaussNewton.t:1056-1092) -- one marching launch per
// iteration in march_pcgIter, 11-16 us each on images that are all launch latency (BASELINE config 1: poisson 256^2).  The protocol is sfs_onchip.h's with a one-pixel ring
// (the sums, their one wait, the q test, alpha / beta are onchip_sync.h's ocGridSum, ocZetaBreak, ocAlpha / ocBeta; this file keeps the tile, Op::apply, which ring words a
// lane asks for and the update over the held rows):
//   tile    a WAVE holds 64 columns x (R + 2) rows of p and r in registers and owns the 62 x R pixels in the middle; the ring is updated by the holder with the owner's
//           alpha, beta and the same fused operations, so the search direction never travels;
//   A p     Op::apply on the owned rows (neighbouring columns: whole-wave DPP shifts; rows above / below: the lane's own registers); flag bit and operator coefficients
//           of the held pixels stay in registers for the whole solve;
//   ring    the A p of a tile's outermost rows / columns goes to a tagged image (8-byte {payload, tag} words, relaxed agent-scope stores, parity-double-buffered) and is
//           picked up by the ring holders inside the ONE wait per iteration that also carries the four sums (alphaNum, alphaDen, s2, s3; beta by expansion as in
//           march_pcgIter, including the reference's start: p_0 = r_0 / 4, alphaNumerator_0 = r_0 . p_0, so sum r_0^2 = 4 alphaNumerator_0 exactly);
//   sums    every workgroup posts its partial sums as tagged words and adds ALL workgroups' words in the same order: the same bits everywhere.
// Every wait is bounded by the device's wall clock; a time-out raises `bad`, nothing is written to delta, the unknowns stay untouched (ocApplyDelta checks the flag) and
// the host redoes the linear solve with the marching kernels.  The grid must be co-resident (one workgroup per CU): the launcher checks workgroups <= CUs.
// Levenberg-Marquardt (LM = true): + CtC p (o.t:2076-2082; CtC as PCGFinalizeDiagonal left it, the start p_0 = M_LM r_0 comes from the solver, later z = r), a fifth sum --
// sum r_0^2 in iteration 0, then Q_k = 1/2 sum delta . (r + b) (solver.t:483-485) formed where iteration k is applied and carried by the sums of iteration k + 1 -- and the
// q early-out (:1093-1102) decided by every workgroup from the same totals.  A residual reset before the last iteration (lIterations > residual_reset_period) keeps the
// solve on the generic kernels by default; with the solver parameter amd_onchip = 2 it takes the kernel's third mode (MODE 2), which does the split reset (:1077-1086,
// kernels :491-534) inside the launch: the wave also keeps delta of its ring pixels, and an iteration k with (k + 1) % residual_reset_period == 0, k + 1 < L ends with a
// second stencil pass A delta, r = b - A delta, z = r and a second grid-wide wait (phase B) that carries sum r.r (beta's numerator) and Q and hands the ring holders the
// new r itself; the zeta test of that iteration is taken right there.  Phases, not iterations, number the tags.  Op::kSplit31 (intrinsic_image_decomposition: two unknown images) only changes where a pixel's scalars sit in the solver's vectors.
#pragma once
#include "stencil_march.h"
#include "onchip_launch.h"

namespace optamd {
namespace {

constexpr int kMoSpan = kWave - 2;            // pixels a wave owns per row (one DPP ring)
constexpr int kMoMaxG = 256;                  // workgroups (one per CU)
constexpr int kMoNSMax = 5, kMoNWMax = 2 * kMoNSMax;   // sums per iteration (Gauss-Newton 4, Levenberg-Marquardt 5); tagged words per workgroup

template <class T>
struct MoArgs {
    OcArgs<T> oc;                           // the protocol's arguments (onchip_launch.h OcGrant::args): the grid, the tags, the tagged buffers, the bounds of the waits, the LM controls
    int W, H;
    const T* r0; const T* p0; T* delta;     // solver vectors: C channels per pixel, interleaved
    const uint8_t* flags; const T* coef;    // Op::kMasked / Op::kCoef
};

// MODE: 0 Gauss-Newton, 1 Levenberg-Marquardt, 2 Levenberg-Marquardt with the split residual reset inside the solve
template <class T, class Op, int R, int WAVES, int MODE>
__global__ __launch_bounds__(WAVES * kWave) void march_onchipPcg(Op op, MoArgs<T> K) {
    constexpr bool LM = MODE != 0, RESET = MODE == 2;
    constexpr int kMoNS = LM ? 5 : 4, kMoNW = 2 * kMoNS;
    constexpr int C = Op::C, HR = R + 2, kBlk = WAVES * kWave, WPS = (int)sizeof(T) / 4;
    constexpr int kCoefN = Op::kCoef > 0 ? Op::kCoef : 1;
    using Vec = MVec<T, C>; using Coef = MVec<T, kCoefN>;
    __shared__ OcSumLds<kMoNS, WAVES, kMoMaxG> sums;
    constexpr bool AP_LDS = C * sizeof(T) * R >= 128;      // where the registers are short, A p of the owned pixels waits in LDS between the stencil and the update: [row][channel][thread]
    __shared__ T apL[AP_LDS ? R * C * kBlk : 1];
    constexpr bool DL_LDS = AP_LDS && Op::kCoef >= 4 && (C + Op::kCoef) * sizeof(T) * R >= 256;      // ... and, for the fattest pixels (four channels + four coefficients), delta itself
    __shared__ T dlL[DL_LDS ? R * C * kBlk : 1];
    __shared__ T bL[LM ? R * C * kBlk : 1];      // LM: b = r_0 of the owned pixels (for Q)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = blockIdx.x;
    const int tile = g * WAVES + wave;
    const int sx = tile % K.oc.stripsX, ty = tile / K.oc.stripsX;
    const bool idle = ty >= K.oc.tilesY;                  // (wave-uniform) a wave without a tile: contributes zeros to the sums
    const int x = sx * kMoSpan + lane - 1;
    const int yBase = ty * R;                          // first owned row; held row h is image row yBase - 1 + h
    const bool xin = !idle && x >= 0 && x < K.W;
    const bool writer = xin && lane >= 1 && lane <= kMoSpan;
    const bool hasL = x >= 1, hasR = x + 1 < K.W;
    const int xc = min(max(x, 0), K.W - 1);
    const int N = K.W * K.H;
    int* const bad = K.oc.bad;
    const long long to = K.oc.timeoutTicks;
    // scalar (pixel i, channel c) of a solver vector: C interleaved channels, or -- Op::kSplit31 -- a 3-channel image followed by a 1-channel image (energy.h)
    auto at = [&](long i, int c) -> long { if constexpr (Op::kSplit31) return c < 3 ? i * 3 + c : 3L * N + i; else return i * C + c; };

    // ---- p_0, r_0, the flag bit and the operator coefficients of the held pixels (a pixel outside the image or switched off: zeros, off); delta = 0 ----------------
    Vec p[HR], r[HR], dl[DL_LDS ? 1 : R], ap[AP_LDS ? 1 : R];
    Coef cf[HR];
    Vec ctc[LM ? R : 1];      // LM: CtC of the owned pixels
    unsigned onBits = 0;
#pragma unroll
    for (int h = 0; h < HR; ++h) {
        const int y = yBase - 1 + h;
        const bool in = xin && y >= 0 && y < K.H;
        const long i = in ? (long)y * K.W + xc : (long)xc;      // a valid address either way
        bool on = in;
        if (Op::kMasked) on = on && (K.flags[i] & 1);
#pragma unroll
        for (int c = 0; c < C; ++c) { const T pv = K.p0[at(i, c)], rv = K.r0[at(i, c)]; p[h].v[c] = on ? pv : T(0); r[h].v[c] = on ? rv : T(0); }
#pragma unroll
        for (int c = 0; c < kCoefN; ++c) cf[h].v[c] = Op::kCoef > 0 ? K.coef[i * kCoefN + c] : T(0);
        onBits |= on ? (1u << h) : 0u;
        if (LM && h >= 1 && h <= R) {
#pragma unroll
            for (int c = 0; c < C; ++c) { const T cv = K.oc.CtC[at(i, c)]; ctc[LM ? h - 1 : 0].v[c] = on ? cv : T(0); bL[((LM ? h - 1 : 0) * C + c) * kBlk + tid] = r[h].v[c]; }      // b = r_0 (solver.t:657)
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) { if (DL_LDS) dlL[((DL_LDS ? i : 0) * C + c) * kBlk + tid] = 0; else dl[DL_LDS ? 0 : i].v[c] = 0; if (AP_LDS) apL[((AP_LDS ? i : 0) * C + c) * kBlk + tid] = 0; else ap[AP_LDS ? 0 : i].v[c] = 0; }

    const int pixBase = (yBase - 1) * K.W + xc;      // index of held row 0 of this lane's column (used only where the row exists)
    auto rowIn = [&](int h) { const int y = yBase - 1 + h; return xin && y >= 0 && y < K.H; };
    bool failed = false;
    double accQ = 0;
    T Q0 = 0;      // fetchQ before the loop (solver.t:1050): delta = 0, so exactly 0
    const size_t boxStride = (size_t)N * C * WPS;
    // RESET: an iteration that ends with the split residual reset (solverGPUGaussNewton.t:1077-1083) takes two trips through this loop, one per grid-wide wait: phase A as
    // ever up to delta += alpha p, then phase B -- a second stencil pass, A delta, with r = b - A delta, z = r, sum r.r and Q, the new r of the tile's outermost rows /
    // columns travelling in the words A p takes otherwise.  Phases, not iterations, number the tags and pick the parity.  State: delta of the ring rows above and below the
    // tile (the side columns' delta is dl of lanes 0 and 63: every lane applies delta += alpha p to the R pixels of its column), the phases passed so far, whether this
    // trip is a phase B, the alpha numerator of its phase A, and whether the Q of the iteration before travels with this trip's sums (after a reset it has been tested).
    Vec dr[RESET ? 2 : 1];
    if constexpr (RESET) {
#pragma unroll
        for (int c = 0; c < C; ++c) { dr[0].v[c] = 0; dr[RESET ? 1 : 0].v[c] = 0; }
    }
    unsigned phase = 0;
    bool phaseB = false, qPending = false;
    T aNumA = 0;

    for (int k = 0; k < K.oc.L; k += phaseB ? 0 : 1) {
        const unsigned tag = K.oc.tag0 + (RESET ? phase : (unsigned)k);
        const int par = (int)(tag & 1u);
        oc_u64* const box = K.oc.apBox + (size_t)par * boxStride;
        oc_u64* const slotPar = K.oc.slots + (size_t)par * K.oc.G * kMoNW;
        if (k == K.oc.failAt && g == 0 && tid == 0) __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool first = k == 0;
        const bool resetIt = RESET && k + 1 < K.oc.L && (k + 1) % K.oc.resetPeriod == 0;      // this iteration ends with the split residual reset: r is formed anew, nobody needs the ring's A p

        // ---- PCGStep1: A p_k on the owned pixels, with the four sums (march_pcgIter's expressions) --------------------------------------------------------------
        double accDen = 0, accNum = 0, acc2 = 0, acc3 = 0, accX = 0;      // accX (LM): sum r_0^2 in iteration 0, the Q of the iteration before in the others
        if constexpr (RESET) {      // ---- phase B: computeAdelta + PCGStep2_2ndHalf (:566-571, 505-534): r = b - (J^T J + CtC) delta, with sum r.r (in accNum) and Q (in accX) ----
            if (phaseB && !idle) {
                auto deltaRow = [&](int h) -> Vec {
                    if (h == 0) return dr[0];
                    if (h == HR - 1) return dr[RESET ? 1 : 0];
                    Vec d;
#pragma unroll
                    for (int c = 0; c < C; ++c) d.v[c] = DL_LDS ? dlL[((DL_LDS ? h - 1 : 0) * C + c) * kBlk + tid] : dl[DL_LDS ? 0 : h - 1].v[c];
                    return d;
                };
                Vec du = deltaRow(0), dc = deltaRow(1);
#pragma unroll
                for (int h = 1; h <= R; ++h) {
                    const int y = yBase - 1 + h;
                    const Vec dd = deltaRow(h + 1);
                    const Vec dlft = marchShift<true>(dc), drgt = marchShift<false>(dc);
                    Vec o = op.apply(dc, dlft, drgt, du, dd, hasL, hasR, y - 1 >= 0, y + 1 < K.H, cf[h]);
                    const bool on = (onBits >> h) & 1u;
#pragma unroll
                    for (int c = 0; c < C; ++c) { o.v[c] += ctc[h - 1].v[c] * dc.v[c]; o.v[c] = on ? o.v[c] : T(0); }
                    if (writer && y < K.H) {
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const T bv = bL[((h - 1) * C + c) * kBlk + tid];
                            const T rn = bv - o.v[c];
                            r[h].v[c] = rn;
                            accNum += (double)rn * (double)rn;
                            accX += (double)(T(0.5) * (dc.v[c] * (rn + bv)));      // solver.t:483-485
                        }
                        if (h == 1 || h == R || lane == 1 || lane == kMoSpan) {
                            const int i = (pixBase + h * K.W) * C;      // (int index: the launcher grants images below 2^30 bytes, OnchipLauncher::plan)
#pragma unroll
                            for (int c = 0; c < C; ++c) ocSend(box, i + c, r[h].v[c], tag);
                        }
                    }
                    du = dc; dc = dd;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (!idle && !(RESET && phaseB)) {
#pragma unroll
            for (int h = 1; h <= R; ++h) {
                const int y = yBase - 1 + h;
                const Vec pl = marchShift<true>(p[h]), pr = marchShift<false>(p[h]);
                Vec o = op.apply(p[h], pl, pr, p[h - 1], p[h + 1], hasL, hasR, y - 1 >= 0, y + 1 < K.H, cf[h]);
                const bool on = (onBits >> h) & 1u;
#pragma unroll
                for (int c = 0; c < C; ++c) { if (LM) o.v[c] += ctc[LM ? h - 1 : 0].v[c] * p[h].v[c]; o.v[c] = on ? o.v[c] : T(0); if (AP_LDS) apL[((AP_LDS ? h - 1 : 0) * C + c) * kBlk + tid] = o.v[c]; else ap[AP_LDS ? 0 : h - 1].v[c] = o.v[c]; }
                if (writer && y < K.H) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const double rr = (double)r[h].v[c], a = (double)o.v[c], pp = (double)p[h].v[c];
                        accNum += (first ? pp : rr) * rr;      // z_0 . r_0 is the reference's r_0 . p_0
                        accDen += pp * a; acc2 += rr * a; acc3 += a * a;
                        if (LM && first) accX += rr * rr;
                    }
                    // the tile's outermost rows / columns: to the tagged image, for whoever holds them as ring
                    if (!resetIt && (h == 1 || h == R || lane == 1 || lane == kMoSpan)) {
                        const int i = (pixBase + h * K.W) * C;      // (int, as above)
#pragma unroll
                        for (int c = 0; c < C; ++c) ocSend(box, i + c, o.v[c], tag);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- the grid-wide sums (onchip_sync.h ocGridSum); the ring's A p (phase B: the ring's new r) is collected inside its ONE wait ---------------------------
        // Ring requests: every lane asks for its column's pixel of the rows above and below the tile; the two side columns are asked for by ONE lane per pixel
        // (lane h: the left neighbour of row h, lane 32 + h: the right one) and handed to lanes 0 / 63 through scalar registers afterwards -- a lane holds three
        // pixels' words during the wait instead of R + 2 (the difference is what lets 16 rows per wave fit).
        static_assert(R + 1 < 32, "one lane per side pixel");
        oc_u64 rw[3][C * WPS];      // top, bottom, side
        {
            if (LM && !first && !(RESET && phaseB)) accX = accQ;
            double part[kMoNS];
            part[0] = accNum; part[1] = accDen; part[2] = acc2; part[3] = acc3;
            if constexpr (LM) part[4] = accX;
            const bool lastIt = k + 1 == K.oc.L || (RESET && resetIt && !phaseB);      // (after the last iteration only delta survives: nobody needs the ring; nor in front of a reset)
            const int sRow = lane & 31, sX = (lane < 32) ? sx * kMoSpan - 1 : sx * kMoSpan + kMoSpan, sY = yBase - 1 + sRow;
            const bool needTop = !lastIt && rowIn(0), needBot = !lastIt && rowIn(HR - 1);
            const bool needSide = !lastIt && !idle && sRow >= 1 && sRow <= R && sX >= 0 && sX < K.W && sY < K.H;
            const size_t iTop = (size_t)pixBase * C * WPS, iBot = (size_t)(pixBase + (HR - 1) * K.W) * C * WPS, iSide = needSide ? ((size_t)sY * K.W + sX) * C * WPS : 0;
            auto askRing = [&]() {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const bool nd = j == 0 ? needTop : j == 1 ? needBot : needSide;
                    const size_t i = j == 0 ? iTop : j == 1 ? iBot : iSide;
#pragma unroll
                    for (int q = 0; q < C * WPS; ++q) rw[j][q] = (oc_u64)tag << 32;
                    if (nd) {
#pragma unroll
                        for (int q = 0; q < C * WPS; ++q) rw[j][q] = ocLoad(box + i + q);
                    }
                }
            };
            auto ringHere = [&]() {
                bool ok = true;
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int q = 0; q < C * WPS; ++q) ok = ok && (unsigned)(rw[j][q] >> 32) == tag;
                return ok;
            };
            ocGridSum(sums, part, tag, slotPar, K.oc.G, bad, k == 0 && !(RESET && phaseB) ? K.oc.firstTicks : to, askRing, ringHere);
        }
        Vec ring[HR];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            ring[0].v[c] = ocPayload<T>(rw[0] + c * WPS); ring[HR - 1].v[c] = ocPayload<T>(rw[1] + c * WPS);
            const T sv = ocPayload<T>(rw[2] + c * WPS);
#pragma unroll
            for (int h = 1; h <= R; ++h) { const T lft = ocReadLane(sv, h), rgt = ocReadLane(sv, 32 + h); ring[h].v[c] = lane == 0 ? lft : rgt; }      // (only lanes 0 and 63 use them)
        }
        const double aNumD = sums.TOT[0], aDenD = sums.TOT[1], s2 = sums.TOT[2], s3 = sums.TOT[3];
        if (sums.gaveUp) { failed = true; break; }      // uniform over the workgroup: a wait timed out somewhere
        if constexpr (RESET) {
            ++phase;
            if (phaseB) {
                if (ocZetaBreak((T)sums.TOT[kMoNS - 1], Q0, k + 1, K.oc.qTolerance, K.oc.lmBreak, k + 2)) break;      // the q test of THIS iteration: the split step delivers Q directly
                const T betaB = (aNumA > T(0)) ? (T)aNumD / aNumA : T(0);      // PCGStep3's guard (:544-547)
                // r as received on the ring, then p = r + beta p everywhere: the bits of the pixel's owner
#pragma unroll
                for (int h = 0; h < HR; ++h) {
                    const bool ownRow = h >= 1 && h <= R;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        if (!(ownRow && writer)) r[h].v[c] = ring[h].v[c];
                        p[h].v[c] = ocFma(betaB, p[h].v[c], r[h].v[c]);
                    }
                }
                qPending = false; accQ = 0; phaseB = false;
                continue;
            }
        }
        if constexpr (LM) {      // the q early-out of iteration k - 1 (solver.t:1093-1102): nothing of iteration k has been applied yet
            if ((RESET ? qPending : !first) && ocZetaBreak((T)sums.TOT[kMoNS - 1], Q0, k, K.oc.qTolerance, K.oc.lmBreak, k + 1)) break;
        }
        // the scalars of march_pcgIter's prologue; the start-up quirk: sum r_0^2 = 4 alphaNumerator_0, exact (LM starts from the preconditioned r_0: sum r_0^2 is summed directly)
        const T alpha = ocAlpha<T>(aNumD, aDenD);
        const T beta = ocBeta<T>(alpha, aNumD, s2, s3, first ? (LM ? sums.TOT[kMoNS - 1] : 4.0 * aNumD) : aNumD);
        const bool last = k + 1 == K.oc.L;

        if constexpr (RESET) {
            if (resetIt) {
                // ---- PCGStep2_1stHalf (solverGPUGaussNewton.t:491-503): delta += alpha p, on the owned pixels and on the ring -------------------------------------------
#pragma unroll
                for (int h = 0; h < HR; ++h) {
                    const bool ownRow = h >= 1 && h <= R;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        if (!ownRow) dr[h == 0 ? 0 : 1].v[c] = ocFma(alpha, p[h].v[c], dr[h == 0 ? 0 : 1].v[c]);
                        else if (DL_LDS) dlL[((DL_LDS && ownRow ? h - 1 : 0) * C + c) * kBlk + tid] = ocFma(alpha, p[h].v[c], dlL[((DL_LDS && ownRow ? h - 1 : 0) * C + c) * kBlk + tid]);
                        else dl[!DL_LDS && ownRow ? h - 1 : 0].v[c] = ocFma(alpha, p[h].v[c], dl[!DL_LDS && ownRow ? h - 1 : 0].v[c]);
                    }
                }
                aNumA = (T)aNumD; phaseB = true;
                continue;
            }
        }

        // ---- PCGStep2 + PCGStep3 (z = r): delta += alpha p;  r -= alpha A p;  p = r + beta p -- on the owned pixels and, with the same fused operations, on the ring
        accQ = 0;
#pragma unroll
        for (int h = 0; h < HR; ++h) {
            const bool ownRow = h >= 1 && h <= R;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const T apv = ownRow ? (writer ? (AP_LDS ? apL[((AP_LDS && ownRow ? h - 1 : 0) * C + c) * kBlk + tid] : ap[!AP_LDS && ownRow ? h - 1 : 0].v[c]) : ring[h].v[c]) : ring[h].v[c];
                T dNew = 0;
                if (RESET && !ownRow && !last) dr[RESET && h != 0 ? 1 : 0].v[c] = ocFma(alpha, p[h].v[c], dr[RESET && h != 0 ? 1 : 0].v[c]);      // (the split residual reset applies A to delta)
                if (ownRow) {
                    dNew = ocFma(alpha, p[h].v[c], DL_LDS ? dlL[((DL_LDS && ownRow ? h - 1 : 0) * C + c) * kBlk + tid] : dl[!DL_LDS && ownRow ? h - 1 : 0].v[c]);
                    if (DL_LDS) dlL[((DL_LDS && ownRow ? h - 1 : 0) * C + c) * kBlk + tid] = dNew; else dl[!DL_LDS && ownRow ? h - 1 : 0].v[c] = dNew;
                }
                if (!last) {
                    r[h].v[c] = ocFma(-alpha, apv, r[h].v[c]);
                    if (LM && ownRow && writer && yBase - 1 + h < K.H) accQ += (double)(T(0.5) * (dNew * (r[h].v[c] + bL[((LM && ownRow ? h - 1 : 0) * C + c) * kBlk + tid])));      // solver.t:483-485
                    p[h].v[c] = ocFma(beta, p[h].v[c], r[h].v[c]);
                }
            }
        }
        if constexpr (RESET) qPending = !last;
    }
    if (failed && tid == 0 && K.oc.hostErr) __hip_atomic_store(K.oc.hostErr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (!failed && writer) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int y = yBase + i;
            if (y < K.H) {
                const long e = (long)y * K.W + x;
#pragma unroll
                for (int c = 0; c < C; ++c) K.delta[at(e, c)] = DL_LDS ? dlL[((DL_LDS ? i : 0) * C + c) * kBlk + tid] : dl[DL_LDS ? 0 : i].v[c];
            }
        }
    }
}

// ---- host side: the family's data for onchip_launch.h ----------------------------------------------------------------------------------------------------------
constexpr OcFamily kMoFamily{kMoSpan, 2, kMoMaxG, kMoNWMax, "march_onchipPcg", "march_pcgIter", "generic kernels", nullptr};

template <class T, class Op, int R, int WV, int MODE> constexpr size_t moLdsBytes() {      // A p and delta (where they wait in LDS) + b (LM, both modes) + the sums' staging
    const size_t plane = (size_t)R * Op::C * sizeof(T) * WV * kWave;
    const bool apLds = Op::C * sizeof(T) * R >= 128, dlLds = apLds && Op::kCoef >= 4 && (Op::C + Op::kCoef) * sizeof(T) * R >= 256;
    return (apLds ? plane : 0) + (dlLds ? plane : 0) + (MODE != 0 ? plane : 0) + 12 * 1024;
}
// a variant whose registers do not hold its loop state is not instantiated (Op::spills, from the compiler's resource remarks); should a compiler upgrade make another one
// spill it is still not offered (hipFuncGetAttributes): no scratch in a kernel that is all latency
template <class T, class Op, int R, int WV, int MODE> const void* moKernel() {
    if constexpr (moLdsBytes<T, Op, R, WV, MODE>() <= 150 * 1024 && !Op::template spills<R, WV, MODE>()) {
        const void* fn = (const void*)march_onchipPcg<T, Op, R, WV, MODE>;
        hipFuncAttributes fa{};
        if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.localSizeBytes == 0) return fn;
        (void)hipGetLastError();
    }
    return nullptr;
}
template <class T, class Op> const std::vector<OcVariant>& moVariants() {
    static const std::vector<OcVariant> v = [] {
        std::vector<OcVariant> o;
#define MO_VARIANT(R, WV) o.push_back({R, WV, moKernel<T, Op, R, WV, 0>(), moKernel<T, Op, R, WV, 1>(), moKernel<T, Op, R, WV, 2>()})
        MO_VARIANT(2, 4); MO_VARIANT(4, 4); MO_VARIANT(8, 4); MO_VARIANT(2, 8); MO_VARIANT(4, 8); MO_VARIANT(8, 8);
        if constexpr (Op::C * sizeof(T) <= 8) { MO_VARIANT(16, 4); MO_VARIANT(16, 8); }
#undef MO_VARIANT
        return o;
    }();
    return v;
}

// ---- a kernel set whose Gauss-Newton PCG loop runs on the marching template (stencil_march.h MarchLoop) and whose whole linear solve goes on chip where it fits:
// the EnergyOps side of both, once.  The kernel set supplies the operator object, the image, its flag image (or none), its enable switch and -- Op::kCoef > 0 --
// the pass that produces the operator's per-pixel coefficients (run on the first launch of a loop and in front of an on-chip solve).
template <class T, class Op, class Base>
struct MarchOps : Base {
    using Base::Base;
    MarchLoop<T> march; OnchipLauncher<T> oc;
    int mW = 0, mH = 0, mCus = 0;
    bool useMarch = true, movableWhenOff = false;      // the enable switch; deltaMovable() with the switch off
    const uint8_t* marchFlags = nullptr;               // Op::kMasked: bit 0 = the pixel is an unknown
    T* coef = nullptr;
    virtual Op marchOp() const = 0;
    virtual void marchCoefficients(T* /*coef*/, LaunchCtx&) {}
    // enableSwitch: the environment variable that switches both paths off (nullptr: none); updateCap: workgroups of the guarded update per unknown image
    void marchInit(int W, int H, int cus, const char* enableSwitch, bool movableOff, long updateCap) {
        mW = W; mH = H; mCus = cus; movableWhenOff = movableOff;
        if (const char* e = enableSwitch ? getenv(enableSwitch) : nullptr) useMarch = atoi(e) != 0;
        oc.init(kMoFamily, moVariants<T, Op>, W, H, Op::C, cus, updateCap);
        if (useMarch) oc.reserve();
    }
    ~MarchOps() override { if (coef) (void)hipFree(coef); }
    void produceCoefficients(LaunchCtx& ctx) {
        if constexpr (Op::kCoef > 0) {
            if (!coef) HIP_CHECK(hipMalloc((void**)&coef, (size_t)Op::kCoef * mW * mH * sizeof(T)));
            ScopedKernel k(ctx, "operatorCoefficients");
            marchCoefficients(coef, ctx);
        }
    }
    bool marched = false;      // the loop in progress runs on the marching template (decided by its first launch)
    bool pcgIteration(const PcgIterArgs<T>& a, LaunchCtx& ctx) override {
        // Gauss-Newton without a preconditioner only; every other loop is Base's business (a functor energy: two launches under amd_stencil_fused = 1, else refused -- the generic kernels)
        if (!useMarch || a.pre || a.CtC) { if (a.first) marched = false; return Base::pcgIteration(a, ctx); }
        if (a.first) { marched = true; produceCoefficients(ctx); }
        return march.launch(marchOp(), mW, mH, marchFlags, mCus, a, ctx, coef);
    }
    const T* pcgFinish(T* delta, LaunchCtx& ctx) override { return marched ? march.finish(delta, (long)Op::C * mW * mH, mCus, ctx) : Base::pcgFinish(delta, ctx); }
    bool deltaMovable() const override { return (useMarch || movableWhenOff) && !this->slab.active; }      // (the march takes delta from its arguments at every launch: PcgSolver::deltaTrial)
    // the whole linear solve on chip, X += delta behind a Gauss-Newton one included (onchip_launch.h)
    bool pcgSolveOnChip(const T* r0, const T* p0, T* delta, int L, double* traceDev, const OnChipLm<T>* lm, LaunchCtx& ctx) override {
        if (!useMarch || traceDev || this->slab.active || !oc.plan(L, lm != nullptr, lm)) return false;      // (asked before the coefficient pass is spent)
        produceCoefficients(ctx);
        return oc.solve(L, lm, delta, *this, ctx, [&](const OcGrant& g) {
            MoArgs<T> K{g.args(L, lm), mW, mH, r0, p0, delta, marchFlags, coef};
            Op op = marchOp();
            void* kargs[] = {(void*)&op, (void*)&K};
            return g.launch(kargs, ctx.stream);
        });
    }
    OnchipGuard* onChipGuard() override { return &oc.guard; }
    // (the loop that is Base's -- Levenberg-Marquardt, or everything with the march switched off -- adds its own note: two launches per PCG iteration or why not)
    std::string describe(int L, bool lmv, const OnChipLm<T>* lmc) override { return oc.describe(useMarch ? L : 0, lmv, lmc) + (lmv || !useMarch ? this->perIterationNote(lmv) : std::string()); }
};

}  // namespace
}  // namespace optamd
