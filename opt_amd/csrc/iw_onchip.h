// image_warping, Gauss-Newton and Levenberg-Marquardt: the WHOLE PCG linear solve as one persistent launch whose loop state never leaves the chip -- on a unit-lattice UrShape
// (iw_onchipPcg, the default) and, for a plan that sets amd_onchip = 4, on any UrShape (iw_onchipPcgGeneral; the kernels share their body, iw_onchip_body.inc).
//
// Included by energy_image_warping.hip (host side: ImageWarpingOps::pcgSolveOnChip).  What it replaces: the reference's loop
// `for lIter = 0, lIterations do PCGStep1; PCGStep2; PCGStep3 end` (solverGPUGaussNewton.t:1056-1092) -- three launches and two same-address-atomic
// sums per iteration there, one streaming launch per iteration in iw_pcgIter2 -- for problems whose state fits the register files and LDS of the
// chip (<= 8192 pixels per CU: 2 M pixels on 256 CUs; the reference's own inputs are 512^2 and 640x480, and 1/8 of the metric's 4096^2 is 4096x512).
// The reference's precedent for an on-chip solve is its block-local comparator (examples/poisson_image_editing/src/PatchSolverWarping.cu:67-196:
// one patch per block, state in shared memory); this kernel is a GLOBAL solve -- the same iterates as the streaming loop -- that keeps
//   p, r            in registers (a lane owns ROWS consecutive rows of one image column),
//   A p             in registers (ROWS <= 8) or LDS (ROWS = 16, 96 KB),
//   delta           in registers, or -- ROWS = 16 -- in the solver's delta vector, read-modify-written once per iteration (the 3 MB per XCD stay in its L2),
//   cos / sin, flag byte of every pixel in registers,
// and synchronises the grid ONCE per iteration with 8-byte {payload, tag} words (one relaxed agent-scope store each, no fences, no cache write-backs;
// MI355X_MICROARCH.md "handoff-1to1" / "allgather"; measured in tools/microbench_gridsync.hip):
//   halo   a workgroup's tile is 256 x 2 ROWS pixels (8 waves: 4 across, 2 down).  Every wave keeps p and r of the one-pixel ring around its pixels itself
//          and receives only the A p of those pixels -- through LDS inside a workgroup, through per-tile inboxes in global memory between workgroups --
//          posted TOGETHER with the partial sums, so the hand-over rides on the wait for the sums (see the kernel's header);
//   sum    the four sums of the iteration (alphaDen = p.Ap, alphaNum = sum M r^2, s2 = sum M r.Ap, s3 = sum M Ap^2; beta by expansion as in iw_pcgIter2,
//          energy.h PcgIterArgs) as a two-level tree: 16 workgroups per group, group totals posted by the group's first workgroup, every workgroup adds the
//          group totals in group order -- the same bits everywhere, so alpha and beta agree on the whole grid without a broadcast.
// Every wait is bounded by the device's wall clock; a time-out raises K.S.bad, every workgroup leaves the loop at its next sum, nothing is applied to the
// unknowns (iw_applyDelta checks the flag) and the host falls back to the streaming loop.  The grid must be co-resident (one workgroup per CU): the launcher
// checks tiles <= CUs x occupancy.
#pragma once
#include "iw_device.h"
#include "onchip_sync.h"

namespace optamd {
namespace {

constexpr int kOcBlock = 512, kOcWavesX = 4, kOcWavesY = 2, kOcWaves = kOcBlock / kWave, kOcTileW = kOcWavesX * kWave;
constexpr int kOcGroup = 16;                  // workgroups per first-level group of the grid-wide sum
constexpr int kOcMaxTiles = 256;              // 16 groups of 16

struct OnchipSync {
    oc_u64* slots;          // [2][G][8]: a workgroup's four double sums as 8 tagged halves
    oc_u64* groupSlots;     // [2][ceil(G / 16)][8]
    oc_u64* inbox;          // [2][G][4 sides][stride]: edge rows / columns of p from the four neighbouring tiles
    int* bad;               // device word: some wait timed out
    int* hostErr;           // pinned host word, set by iw_applyDelta when `bad` is
    long stride;            // words per (tile, side): 3 * kOcTileW scalars
};
// Row slabs (one rank per GPU): the links of this rank's kernel to the other ranks' (include/OptAmd.h OptAmd_OnChipLinks; world <= 1: none).
struct OcLinks {
    oc_u64* mailDst[16]; const oc_u64* mailMine;
    int world, rank, slots, slotStride, rankStride; unsigned seq0;
    oc_u64 *edgeSendUp, *edgeSendDown; const oc_u64 *edgeRecvUp, *edgeRecvDown; long edgeParityStride;
};
template <class T>
struct OnchipArgs {
    int W, H, tilesX, tilesY, G;        // H: rows of the arrays (a slab's include its ghost rows)
    int yBegin, yEnd;                   // the rows the tiles cover: [0, H) on one GPU, the slab's owned rows (a multiple of the tile height) otherwise
    OcLinks links;
    const T* r0; const T* p0;           // solver layout: [O.x O.y] x N, then [a] x N
    const T* Angle; const uint8_t* flags;
    T* delta;                           // out: sum alpha_k p_k
    T w_fit, w_reg;
    int L; unsigned tag0;               // iterations; tag of iteration 0 (tags never repeat over the life of the buffers)
    int flat;                           // 1: every workgroup reads every workgroup's slot (small grids); 0: two-level tree
    OnchipSync S;
    double* trace;                      // [L][4] = alphaNum, alphaDen, s2, s3 of every iteration (written by workgroup 0), or nullptr
    long long timeoutTicks;
    long long firstTicks;               // bound of the waits of the FIRST phase: passing it proves that every workgroup of the grid is resident (each has posted its words), so it is the
                                        // co-residency check -- short (10 ms), before anything has been written; row slabs: = timeoutTicks (the first sum waits for the other ranks' launches)
    long long* prof;                    // OC_PROFILE builds: [G][8] ticks per phase, else nullptr
    int failAt;                         // test hook (OPT_AMD_ONCHIP_FAIL_AT): workgroup 0 raises `bad` in this iteration as a timed-out wait would; -1: never
    // Levenberg-Marquardt variants (LMV): the scalars of PCGFinalizeDiagonal (solver.t:631-664), the q early-out and the residual reset period (:1077-1102)
    T lmRadius, lmMin, lmMax, qTolerance; int resetPeriod;      // (LMV: `trace` is the pinned {iteration + 1, zeta} word of the q early-out instead, OnChipLm::breakInfo -- the LM variants are never traced)
    // General UrShape (iw_onchipPcgGeneral; unread by the unit-lattice kernels): the rest shape, the solver's Jacobi preconditioner vector (its Angle channel is read: PCGInit1's
    // guardedInvert(diag), or PCGFinalizeDiagonal's LM preconditioner) and, LMV, its CtC vector (Angle channel) -- solver layout
    const T* UrShape; const T* pre; const T* CtC;
};

// one scalar of the halo as tagged words (a float is one word, a double two): sent with onchip_sync.h's ocSend
__device__ __forceinline__ void ocRecv(const oc_u64* box, int idx, unsigned tag, int* bad, long long to, float& v) { v = __uint_as_float(ocAwait(box + idx, tag, bad, to)); }
__device__ __forceinline__ void ocRecv(const oc_u64* box, int idx, unsigned tag, int* bad, long long to, double& v) {
    const unsigned lo = ocAwait(box + 2 * idx, tag, bad, to), hi = ocAwait(box + 2 * idx + 1, tag, bad, to);
    v = __longlong_as_double((long long)(((oc_u64)hi << 32) | lo));
}
// Three scalars of one halo pixel at once: all requests are in flight together (one fabric round trip when the words are already there, not three).
template <bool SYS = false> __device__ __forceinline__ void ocRecv3(const oc_u64* box, int i0, int i1, int i2, unsigned tag, int* bad, long long to, float (&v)[3]) {
    const oc_u64 *p0 = box + i0, *p1 = box + i1, *p2 = box + i2;
    oc_u64 a = ocLoad<SYS>(p0), b = ocLoad<SYS>(p1), c = ocLoad<SYS>(p2);
    if ((unsigned)(a >> 32) != tag || (unsigned)(b >> 32) != tag || (unsigned)(c >> 32) != tag) {
        const long long t0 = wall_clock64();
        unsigned spins = 0;
        for (;;) {
            __builtin_amdgcn_s_sleep(1);
            a = ocLoad<SYS>(p0); b = ocLoad<SYS>(p1); c = ocLoad<SYS>(p2);
            if ((unsigned)(a >> 32) == tag && (unsigned)(b >> 32) == tag && (unsigned)(c >> 32) == tag) break;
            if ((++spins & 31u) == 0) {
                if (__hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (wall_clock64() - t0 > to) { __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
        }
    }
    v[0] = __uint_as_float((unsigned)a); v[1] = __uint_as_float((unsigned)b); v[2] = __uint_as_float((unsigned)c);
}
template <bool SYS = false> __device__ __forceinline__ void ocRecv3(const oc_u64* box, int i0, int i1, int i2, unsigned tag, int* bad, long long to, double (&v)[3]) {
    const oc_u64* q[6] = {box + 2 * i0, box + 2 * i0 + 1, box + 2 * i1, box + 2 * i1 + 1, box + 2 * i2, box + 2 * i2 + 1};
    oc_u64 w[6];
    auto fetch = [&]() { bool ok = true; for (int i = 0; i < 6; ++i) w[i] = ocLoad<SYS>(q[i]); for (int i = 0; i < 6; ++i) ok = ok && (unsigned)(w[i] >> 32) == tag; return ok; };
    if (!fetch()) {
        const long long t0 = wall_clock64();
        unsigned spins = 0;
        for (;;) {
            __builtin_amdgcn_s_sleep(1);
            if (fetch()) break;
            if ((++spins & 31u) == 0) {
                if (__hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (wall_clock64() - t0 > to) { __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
        }
    }
    for (int i = 0; i < 3; ++i) v[i] = __longlong_as_double((long long)((w[2 * i + 1] << 32) | (w[2 * i] & 0xffffffffull)));
}

// Whole-wave shifts that KEEP `old` in the lane whose source lies outside the wave (bound_ctrl off): lane 0 of fromLeft / lane 63 of fromRight receive the
// halo value the caller put there, every other lane its neighbour's register -- the wave-edge column costs no extra instruction.
__device__ __forceinline__ int ocFromLeft(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ int ocFromRight(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ float ocFromLeft(float old, float v) { return __int_as_float(ocFromLeft(__float_as_int(old), __float_as_int(v))); }
__device__ __forceinline__ float ocFromRight(float old, float v) { return __int_as_float(ocFromRight(__float_as_int(old), __float_as_int(v))); }
__device__ __forceinline__ double ocFromLeft(double old, double v) {
    return __hiloint2double(ocFromLeft(__double2hiint(old), __double2hiint(v)), ocFromLeft(__double2loint(old), __double2loint(v)));
}
__device__ __forceinline__ double ocFromRight(double old, double v) {
    return __hiloint2double(ocFromRight(__double2hiint(old), __double2hiint(v)), ocFromRight(__double2loint(old), __double2loint(v)));
}

template <class T> struct __attribute__((aligned(16))) OcH4 { T v[4]; };      // {ox, oy, a, -} of p, r or A p, or {cos, sin, on, flag byte} of one halo pixel

// LDS carve-up (bytes), shared by the kernel and the launcher
constexpr int kOcSumsMax = 6;                 // capacity of the per-phase sums (Gauss-Newton 4, Levenberg-Marquardt 5)
template <class T> struct OcLds {
    static constexpr size_t ap(int rows, bool apLds) { return apLds ? (size_t)rows * 3 * kOcBlock * sizeof(T) : 0; }
    static constexpr size_t row() { return (size_t)kOcWaves * 2 * 3 * kWave * sizeof(T); }
    static constexpr size_t rows3(bool apLds) { return (apLds ? 2 : 3) * row(); }      // p and r of the halo rows; their A p only when it cannot be read from apL
    static constexpr size_t side(int rows) { return (size_t)kOcWaves * rows * 2 * sizeof(OcH4<T>); }
    static constexpr size_t tail() { return (kOcSumsMax * kOcWaves + kOcGroup * kOcSumsMax + 8) * sizeof(double) + (kOcMaxTiles * 2 * kOcSumsMax + kOcGroup * 8) * sizeof(unsigned) + 32 * sizeof(T) + 16; }
    // Levenberg-Marquardt: b = r_0 of the lane's pixels ([row][component][thread], like apL), delta of the halo rows and of the halo columns
    static constexpr size_t lm(int rows) { return ap(rows, true) + row() + side(rows); }
    // cos / sin of the lane's LAST csRows rows live in LDS instead of registers where that relieves a variant that spills and the LDS has the room: the LM ROWS = 8 variant
    // (round 6: 124 -> 68-76 B of scratch per lane; a row's pair is read back once per stencil pass): [row][cos, sin][thread], behind everything else.  (ROWS = 16 has no room: its
    // A p fills 96 of the CU's 160 KB and the rest is taken to within 6 KB; its 40 B of scratch stay -- ~13 scratch operations per iteration of ~2000 VALU instructions.)
    static constexpr int csRows(int rows, bool apLds, bool lmv) { return (sizeof(T) == 4 && rows == 8 && lmv && !apLds) ? 8 : 0; }
    static constexpr size_t base(int rows, bool apLds, bool lmv) { return ap(rows, apLds) + rows3(apLds) + 5 * side(rows) + tail() + (lmv ? lm(rows) : 0); }
    static constexpr size_t total(int rows, bool apLds, bool lmv = false) { return base(rows, apLds, lmv) + (size_t)csRows(rows, apLds, lmv) * 2 * kOcBlock * sizeof(T); }
    // General UrShape (iw_onchipPcgGeneral): {ux, uy, M_a, -} of the halo columns, one record per pixel beside sideC -- behind everything else, so that no offset of the
    // unit-lattice layout moves.  (The lane's own U, M_a and CtC_a and those of the halo rows are lane-aligned and live in registers; in LDS they would take 57 KB where the
    // double LM variant has 20 left.)
    static constexpr size_t general(int rows) { return side(rows); }
    static constexpr size_t totalGeneral(int rows, bool lmv) { return total(rows, false, lmv) + general(rows); }
};

// Development builds (opt_amd/build.py build_variant with OC_PROFILE=1; tools/onchip_bench.py under OPT_AMD_ONCHIP_PROFILE=1): thread 0 of every workgroup
// accumulates the wall-clock ticks (100 MHz) it spends in each phase of an iteration and leaves them in K.prof[workgroup][8].
#ifndef OC_PROFILE
#define OC_PROFILE 0
#endif
#if OC_PROFILE
#define OC_MARK(i) do { if (lane == 0) { const long long t_ = wall_clock64(); ocProf[wave * 16 + (i)] += t_ - ocPrev; ocPrev = t_; } } while (0)
#else
#define OC_MARK(i) do { } while (0)
#endif

// ONE grid-wide wait per iteration.  A tile keeps p and r of its own pixels AND of the one-pixel ring around every wave (rows above / below: registers, lane-aligned;
// columns left / right: LDS, one lane per halo pixel).  After the stencil a wave hands the A p of its edge pixels to whoever holds them as halo -- the neighbouring
// wave through LDS, the neighbouring tile through its inbox -- together with the workgroup's partial sums; after the one wait everybody applies PCGStep2 / PCGStep3
// to its own pixels and to its halo copies with the same alpha, beta and the same explicitly fused operations: owner and halo holder get the same bits, and the
// new search direction never has to travel.
//
// LMV: the Levenberg-Marquardt loop (solverGPUGaussNewton.t:1056-1103 with the LM branches) in the same protocol:
//   * A = J^T J + diag(CtC) (o.t:2076-2082); CtC and the LM preconditioner of PCGFinalizeDiagonal (:631-664) are 15-entry tables indexed by the flag byte, as in
//     iw_pcgIter2<.., LM> (on a unit lattice diag(J^T J) is a function of the flag byte, and SSq = guardedInvert(diag) never changes);
//   * Q_k = 1/2 sum delta . (r + b) (:483-485) is formed where PCGStep2 updates delta and r -- behind the wait of iteration k -- and travels with the sums of
//     iteration k + 1: the zeta test of iteration k (:1093-1102) is decided by EVERY workgroup from the same five totals at the wait of iteration k + 1, before
//     anything of iteration k + 1 has been applied, so an early-out leaves exactly the reference's delta (its last PCGStep3 is dead);
//   * every residual_reset_period-th iteration ends with the split PCGStep2 (:1077-1083, 491-534): delta += alpha p, then a SECOND stencil pass A delta with its own
//     hand-over and grid-wide wait (phase B), r = b - A delta, z = M r, beta = sum z.r / alphaNumerator, Q directly.  Halo holders keep delta of their ring
//     pixels as well, and the second pass hands them the new r of the edge pixels in the words the first pass uses for A p.
// Phases (not iterations) number the tags and select the parity of the double-buffered boxes: a workgroup can pass the wait of phase n + 1 only after every
// workgroup has read its phase-n words.
//
// LATTICE = false (iw_onchipPcgGeneral): UrShape is an arbitrary input array (image_warping.t:4).  Protocol, tile shape, sums, hand-over, LM phases and time-outs are the same; the
// pairs are evaluated with U_c - U_n read from the pixels' records (iw_pairQ / iw_pairFull<.., false>) and the Angle channel of the preconditioner -- and of CtC -- is no function
// of the flag byte any more: M_a = guardedInvert(sum over the active pairs of (w D)^2) depends on U and, through D = R'(a) dU, on nothing else that changes during the solve.  A halo
// holder cannot rebuild it (a ring pixel's diagonal involves pixels two out), so nobody does: U, M_a and CtC_a are read ONCE at entry -- M_a and CtC_a from the vectors PCGInit1 /
// PCGFinalizeDiagonal have just written, the streaming general loop's values bit for bit -- and kept beside the other per-pixel constants: in registers like cos / sin for the
// lane's pixels and the halo rows, in LDS beside sideC for the halo columns (OcLds::general).  The Offset channel
// keeps its tables.  U travels through the same DPP shifts as cos / sin.
template <class T, int ROWS, bool AP_LDS, bool DELTA_GLB, bool LMV = false>
__global__ __launch_bounds__(kOcBlock, 2) void iw_onchipPcg(OnchipArgs<T> K) {
    constexpr bool LATTICE = true;
#include "iw_onchip_body.inc"
}
// The same solve for a general UrShape (amd_onchip >= 4): A p and delta in registers
template <class T, int ROWS, bool LMV>
__global__ __launch_bounds__(kOcBlock, 2) void iw_onchipPcgGeneral(OnchipArgs<T> K) {
    constexpr bool LATTICE = false, AP_LDS = false, DELTA_GLB = false;
#include "iw_onchip_body.inc"
}

// Behind an on-chip Levenberg-Marquardt solve (whose update the solver applies itself: savePreviousUnknowns + PCGLinearUpdate): tell the host if a wait timed out.
__global__ void iw_relayBad(const int* __restrict__ bad, int* hostErr) {
    if (threadIdx.x == 0 && __hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(hostErr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// PCGLinearUpdate X += delta (solver.t:552-557) behind the on-chip solve -- unless one of its waits timed out: then the unknowns stay untouched, the host is
// told (pinned word) and redoes the linear solve with the streaming kernels.  Row slabs: `verdict` is the all-reduced count of ranks whose kernel failed, so
// either every rank applies its delta or none does.
template <class T>
__global__ __launch_bounds__(kBlock) void iw_applyDelta(T* __restrict__ XO, T* __restrict__ XA, const T* __restrict__ delta, long N, const int* __restrict__ bad,
                                                        const double* __restrict__ verdict, int* hostErr, int* stepErr = nullptr) {
    const bool fail = verdict ? verdict[0] != 0.0 : __hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    if (fail) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            __hip_atomic_store(hostErr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (stepErr) __hip_atomic_store(stepErr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // (OnchipGuard::setStepSlot: which of several enqueued steps this was)
        }
        return;
    }
    V2<T>* xO = (V2<T>*)XO; const V2<T>* dO = (const V2<T>*)delta;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        const V2<T> xv = xO[i], dv = dO[i];
        xO[i] = V2<T>{xv.x + dv.x, xv.y + dv.y};
        XA[i] = XA[i] + delta[2 * N + i];
    }
}
// a rank's own verdict as the double the communicator all-reduces (row slabs)
__global__ void iw_badToScalar(const int* __restrict__ bad, int force, double* out) {
    if (threadIdx.x == 0) out[0] = (force || __hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 1.0 : 0.0;
}

}  // namespace
}  // namespace optamd
