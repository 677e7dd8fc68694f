// arap_mesh_deformation (and volumetric_mesh_deformation on ARAP's kernels) on a SMALL symmetric graph: the WHOLE PCG linear solve of a Gauss-Newton or Levenberg-Marquardt
// step as ONE launch of ONE workgroup (solver parameter amd_onchip = 5).  Included by energy_graph.hip behind the plane gather it mirrors.
//
// What it replaces: two launches per PCG iteration, arap_flatStepPlanes + arap_applyEll (ArapOps::pcgIteration).  The reference's own meshes have 130 - 2000 vertices
// (examples/arap_mesh_deformation: small_armadillo.ply, 386 vertices after one subdivision, 20 x 100 PCG iterations per pass): each of those launches touches a few
// kilobytes, so an iteration costs two dependent dispatches and nothing else.  Here all of the problem sits in one compute unit:
//   p       the search direction of every vertex in LDS, as the dynamic planes D0 / D1 of the streaming path ({p.x, p.y, p.z, pa.x}, {pa.y, pa.z}): a neighbour's p is an
//           LDS read, the vertex's own too;
//   delta   in LDS in the same layout: the split residual reset gathers A delta from it;
//   r, A p (and M where the registers allow) of a lane's V vertices in registers; vertex s * blockDim + tid is slot s of thread tid, so the ELL lists, the static
//           planes T0 / T1 / U0 of this Gauss-Newton step (arap_buildStatic) and the solver's vectors are read coalesced; b, CtC (LM) and the static planes are re-read
//           from memory where they are used: a few kilobytes that stay in the CU's cache;
//   A p     the gather of arap_applyEll over the same planes and ELL out-lists, the same expressions in the same order per vertex: both kernels include
//           arap_half_edge_pair.inc for the walk's body, and differ only in where a neighbour's p comes from;
//   sums    formed in double; wave sum (ocWaveSum63), one partial per wave in LDS, every lane adds the partials in wave order (onchip_sync.h ocWorkgroupSum): the same bits in
//           every lane, in every run.
// The iterates are those of the two-kernel loop -- its terms of the sums (graph_pcg.h iterTerm), its alpha and beta (ocAlpha, ocBeta: the values of
// graph_flat_scalars.inc) -- only the order of the sums differs, which is why the path is opt-in.  Two pieces remain COPIES of the streaming kernels' text, not shared
// with them: the centred part at the end of aoApply (arap_applyEll's, arap_applyFused's) and the per-scalar update of the step (arap_flatStepPlanes'); as functions they
// changed the streaming kernels' instructions (profiles/graph_shared_text.md).  A change to either has to be made in every copy;
// tests/test_onchip_arap_gpu.py::test_same_iterates_as_the_two_kernel_loop is what notices a copy that drifts.
// Levenberg-Marquardt: A = J^T J + diag(CtC), b = r_0, Q = 1/2 sum delta . (r + b) carried
// by the next iteration's sums, the q early-out (onchip_sync.h ocZetaBreak), and the split residual reset (solverGPUGaussNewton.t:1077-1086) as a second gather pass A delta
// at every residual_reset_period-th iteration -- inside one workgroup that costs a barrier.
// Synchronisation: __syncthreads and nothing else.  No polling loop, no tagged word, no co-residency requirement, no time-out path; every break is decided from totals
// that are the same bits in every lane, so every barrier is reached by every wave.
#pragma once
#include "graph_pcg.h"
#include "onchip_sync.h"

namespace optamd {
namespace {

constexpr int kAoMaxWaves = kOcWgMaxWaves, kAoMaxBlock = kOcWgMaxBlock;      // one workgroup of up to 512 threads: 2 waves per SIMD, 256 registers per lane (at 1024 threads and 128 registers every variant spilled)
template <class T> struct alignas(2 * sizeof(T)) AoP2 { T a, b; };
// lanes keep M in registers where V vertices' r, A p, delta and M fit the 128 registers; else M is re-read where it is used
template <class T, int V> constexpr bool aoKeepsM() { return V * sizeof(T) <= 8; }
// neighbours of a vertex in flight together: as many as the registers hold without scratch
template <class T, int V, bool LMV> constexpr int aoBatch() { return sizeof(T) == 4 ? (V == 1 ? 3 : 2) : (V == 1 ? 2 : 1); }
template <class T> constexpr size_t aoLdsPerVertex() { return 2 * (sizeof(Q4<T>) + sizeof(AoP2<T>)); }      // p and delta

template <class T>
struct ArapOcArgs {
    ArapArgs<T> A;                  // N, Constraints, w_fit, w_reg
    ArapPlanes<T> P;                // T0, T1, U0 of this Gauss-Newton step, the ELL out-lists, deg, K
    const T* r0; const T* p0; const T* M; T* delta;
    int L; double* trace;           // 4 doubles per iteration (alphaNum, alphaDen, s2, s3), or nullptr
    const T* CtC; T qTolerance; int resetPeriod; double* lmBreak;      // Levenberg-Marquardt
};

// (J^T J v)(i) [+ CtC v] of vertex i from its own v = (pv, pav) and the neighbours' v in LDS: arap_applyEll's walk.  acc += v(i) . out
template <class T, int BATCH, bool LMV>
__device__ __forceinline__ void aoApply(const ArapOcArgs<T>& K, const Q4<T>* __restrict__ L0, const AoP2<T>* __restrict__ L1, long i, bool ok, int deg, int dmax, T wf,
                                        const V3<T>& pv, const V3<T>& pav, V3<T>& oO, V3<T>& oA, double& acc) {
    const long N = K.A.N, iv = ok ? i : 0;
    const ArapPlanes<T>& P = K.P;
    const T w = K.A.w_reg;
    const Q4<T> t0 = P.T0[iv], t1 = P.T1[iv], u0 = P.U0[iv];
    const ArapCoef<T> cv = arap_coef(t0.a, t0.b, t0.c, t0.d, t1.a, t1.b);
    T s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
    for (int j0 = 0; j0 < dmax; j0 += BATCH) {
        int nid[BATCH]; T wm[BATCH];
        Q4<T> nd0[BATCH], nt0[BATCH], nt1[BATCH], nu0[BATCH]; AoP2<T> nd1[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) { const int jj = j0 + j; wm[j] = jj < deg ? w : T(0); nid[j] = P.ell[(long)min(jj, P.K - 1) * N + iv]; }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) { nd0[j] = L0[nid[j]]; nd1[j] = L1[nid[j]]; nt0[j] = P.T0[nid[j]]; nt1[j] = P.T1[nid[j]]; nu0[j] = P.U0[nid[j]]; }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
#include "arap_half_edge_pair.inc"
        }
    }
    // per-vertex ("centred") part: fitting term and, for LM, CtC p
    V3<T> q{wf * wf * pv.x, wf * wf * pv.y, wf * wf * pv.z}, qa{0, 0, 0};
    if (LMV) { const V3<T> cO = ldv3(K.CtC, iv), cA = ldv3(K.CtC + 3 * N, iv); q.x += cO.x * pv.x; q.y += cO.y * pv.y; q.z += cO.z * pv.z; qa.x = cA.x * pav.x; qa.y = cA.y * pav.y; qa.z = cA.z * pav.z; }
    if (ok) acc += (double)(dot3(pv, q) + dot3(pav, qa));
    oO = V3<T>{q.x + s0, q.y + s1, q.z + s2}; oA = V3<T>{qa.x + s3, qa.y + s4, qa.z + s5};
}

template <class T, int V, bool LMV>
__global__ __launch_bounds__(kAoMaxBlock) void arap_onchipPcg(ArapOcArgs<T> K) {
    constexpr int NS = LMV ? 5 : 4, BATCH = aoBatch<T, V, LMV>();
    constexpr bool MREG = aoKeepsM<T, V>();
    extern __shared__ __align__(16) unsigned char aoLds[];
    __shared__ __align__(16) double red[NS * kAoMaxWaves];
    __shared__ __align__(16) double red2[2 * kAoMaxWaves];
    const int tid = threadIdx.x, nT = blockDim.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), nW = nT >> 6;
    const long N = K.A.N, offA = 3 * N;
    const size_t cap = (size_t)nT * V;
    // p and delta of every vertex as planes {x, y, z, a.x}, {a.y, a.z}: a lane reads and writes its own vertices' entries, the gathers read the neighbours'
    Q4<T>* const L0 = reinterpret_cast<Q4<T>*>(aoLds); Q4<T>* const DL0 = L0 + cap;
    AoP2<T>* const L1 = reinterpret_cast<AoP2<T>*>(DL0 + cap); AoP2<T>* const DL1 = L1 + cap;
    for (int e = tid; e < NS * kAoMaxWaves; e += nT) red[e] = 0.0;
    for (int e = tid; e < 2 * kAoMaxWaves; e += nT) red2[e] = 0.0;

    V3<T> rO[V], rA[V], mO[MREG ? V : 1], mA[MREG ? V : 1];
    T wf[V]; int deg[V], dmax[V]; bool ok[V];
#pragma unroll
    for (int s = 0; s < V; ++s) {
        const long i = (long)s * nT + tid;
        ok[s] = i < N;
        const long iv = ok[s] ? i : 0;
        const V3<T> z3{0, 0, 0};
        rO[s] = ok[s] ? ldv3(K.r0, iv) : z3; rA[s] = ok[s] ? ldv3(K.r0 + offA, iv) : z3;
        const V3<T> pO = ok[s] ? ldv3(K.p0, iv) : z3, pA = ok[s] ? ldv3(K.p0 + offA, iv) : z3;
        if (MREG) { mO[MREG ? s : 0] = ok[s] ? ldv3(K.M, iv) : z3; mA[MREG ? s : 0] = ok[s] ? ldv3(K.M + offA, iv) : z3; }
        wf[s] = (ok[s] && K.A.Constraints[3 * iv] >= T(-999999.9)) ? K.A.w_fit : T(0);
        deg[s] = ok[s] ? K.P.deg[iv] : 0;
        int dm = deg[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dm = max(dm, __shfl_xor(dm, o, kWave));      // the wave walks as many slots as its longest list
        dmax[s] = dm;
        L0[i] = Q4<T>{pO.x, pO.y, pO.z, pA.x}; L1[i] = AoP2<T>{pA.y, pA.z};
        DL0[i] = Q4<T>{T(0), T(0), T(0), T(0)}; DL1[i] = AoP2<T>{T(0), T(0)};
    }
    auto loadM = [&](int s, V3<T>& o, V3<T>& a) {
        if (MREG) { o = mO[MREG ? s : 0]; a = mA[MREG ? s : 0]; }
        else { const long i = (long)s * nT + tid; const V3<T> z3{0, 0, 0}; o = ok[s] ? ldv3(K.M, i) : z3; a = ok[s] ? ldv3(K.M + offA, i) : z3; }
    };
    auto loadB = [&](int s, V3<T>& o, V3<T>& a) {      // b = r_0 (solver.t:657)
        const long i = (long)s * nT + tid; const V3<T> z3{0, 0, 0};
        o = ok[s] ? ldv3(K.r0, i) : z3; a = ok[s] ? ldv3(K.r0 + offA, i) : z3;
    };
    // delta += alpha p of slot s (PCGStep2's first half, solver.t:461-462); returns the new delta
    auto addToDelta = [&](int s, T alpha, const V3<T>& pO, const V3<T>& pA, V3<T>& dO, V3<T>& dA) {
        const long i = (long)s * nT + tid;
        const Q4<T> e0 = DL0[i]; const AoP2<T> e1 = DL1[i];
        dO = V3<T>{e0.a + alpha * pO.x, e0.b + alpha * pO.y, e0.c + alpha * pO.z};
        dA = V3<T>{e0.d + alpha * pA.x, e1.a + alpha * pA.y, e1.b + alpha * pA.z};
        DL0[i] = Q4<T>{dO.x, dO.y, dO.z, dA.x}; DL1[i] = AoP2<T>{dA.y, dA.z};
    };

    double accQ = 0;
    T Q0 = 0;                 // fetchQ before the loop (solver.t:1050): delta = 0, so exactly 0
    bool qPending = false;    // LM: the Q of the iteration before travels with this iteration's sums
    for (int k = 0; k < K.L; ++k) {
        __syncthreads();      // every vertex's p is in LDS
        // ---- PCGStep1: A p_k with the sums of the expanded beta numerator (arap_applyEll with S.r) ----
        double sums[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) sums[q] = 0;
        V3<T> aO[V], aA[V];
#pragma unroll
        for (int s = 0; s < V; ++s) {
            const long i = (long)s * nT + tid;
            const Q4<T> d0 = L0[i]; const AoP2<T> d1 = L1[i];
            const V3<T> pv{d0.a, d0.b, d0.c}, pav{d0.d, d1.a, d1.b};
            aoApply<T, BATCH, LMV>(K, L0, L1, i, ok[s], deg[s], dmax[s], wf[s], pv, pav, aO[s], aA[s], sums[1]);
            if (ok[s]) {
                V3<T> mo, ma; loadM(s, mo, ma);
                const V3<T>&ro = rO[s], &ra = rA[s], &oO = aO[s], &oA = aA[s];
                sums[0] += iterTerm(mo.x, ro.x, ro.x) + iterTerm(mo.y, ro.y, ro.y) + iterTerm(mo.z, ro.z, ro.z) + iterTerm(ma.x, ra.x, ra.x) + iterTerm(ma.y, ra.y, ra.y) + iterTerm(ma.z, ra.z, ra.z);
                sums[2] += iterTerm(mo.x, ro.x, oO.x) + iterTerm(mo.y, ro.y, oO.y) + iterTerm(mo.z, ro.z, oO.z) + iterTerm(ma.x, ra.x, oA.x) + iterTerm(ma.y, ra.y, oA.y) + iterTerm(ma.z, ra.z, oA.z);
                sums[3] += iterTerm(mo.x, oO.x, oO.x) + iterTerm(mo.y, oO.y, oO.y) + iterTerm(mo.z, oO.z, oO.z) + iterTerm(ma.x, oA.x, oA.x) + iterTerm(ma.y, oA.y, oA.y) + iterTerm(ma.z, oA.z, oA.z);
            }
        }
        if constexpr (LMV) sums[NS - 1] = accQ;
        ocWorkgroupSum<NS>(sums, red, lane, wave, nW);
        if (K.trace && tid == 0) { K.trace[4 * k] = sums[0]; K.trace[4 * k + 1] = sums[1]; K.trace[4 * k + 2] = sums[2]; K.trace[4 * k + 3] = sums[3]; }
        if constexpr (LMV) {      // the q early-out of iteration k - 1 (solver.t:1093-1102): nothing of iteration k has been applied yet
            if (qPending && ocZetaBreak((T)sums[NS - 1], Q0, k, K.qTolerance, K.lmBreak, k + 1)) break;
        }
        const T alpha = ocAlpha<T>(sums[0], sums[1]);
        const T beta = ocBeta<T>(alpha, sums[0], sums[2], sums[3], sums[0]);
        const bool last = k + 1 == K.L;      // after the last iteration only delta survives
        if (last || (LMV && K.resetPeriod > 0 && (k + 1) % K.resetPeriod == 0)) {
#pragma unroll
            for (int s = 0; s < V; ++s) {
                const long i = (long)s * nT + tid;
                const Q4<T> d0 = L0[i]; const AoP2<T> d1 = L1[i];
                V3<T> dO, dA;
                addToDelta(s, alpha, V3<T>{d0.a, d0.b, d0.c}, V3<T>{d0.d, d1.a, d1.b}, dO, dA);
            }
            if (last) break;
        }
        if constexpr (LMV) {
            if (K.resetPeriod > 0 && (k + 1) % K.resetPeriod == 0) {
                // ---- the split residual reset (solver.t:1077-1083) behind delta += alpha p: r = b - (J^T J + CtC) delta; z = M r; sum r . z and Q directly ----
                __syncthreads();      // every vertex's delta is in LDS
                double two[2] = {0, 0}, unused = 0;
#pragma unroll
                for (int s = 0; s < V; ++s) {
                    const long i = (long)s * nT + tid;
                    const Q4<T> e0 = DL0[i]; const AoP2<T> e1 = DL1[i];
                    const V3<T> dO{e0.a, e0.b, e0.c}, dA{e0.d, e1.a, e1.b};
                    V3<T> AdO, AdA;
                    aoApply<T, BATCH, LMV>(K, DL0, DL1, i, ok[s], deg[s], dmax[s], wf[s], dO, dA, AdO, AdA, unused);
                    V3<T> bo, ba, mo, ma; loadB(s, bo, ba); loadM(s, mo, ma);
                    rO[s] = V3<T>{bo.x - AdO.x, bo.y - AdO.y, bo.z - AdO.z}; rA[s] = V3<T>{ba.x - AdA.x, ba.y - AdA.y, ba.z - AdA.z};
                    if (ok[s]) {      // k_step2SecondHalf's sums, scalar by scalar
                        const T rr[6] = {rO[s].x, rO[s].y, rO[s].z, rA[s].x, rA[s].y, rA[s].z}, mm[6] = {mo.x, mo.y, mo.z, ma.x, ma.y, ma.z};
                        const T bb[6] = {bo.x, bo.y, bo.z, ba.x, ba.y, ba.z}, dd[6] = {dO.x, dO.y, dO.z, dA.x, dA.y, dA.z};
#pragma unroll
                        for (int c = 0; c < 6; ++c) { const T zz = mm[c] * rr[c]; two[0] += (double)(zz * rr[c]); two[1] += (double)(T(0.5) * (dd[c] * (rr[c] + bb[c]))); }
                    }
                }
                ocWorkgroupSum<2>(two, red2, lane, wave, nW);
                if (ocZetaBreak((T)two[1], Q0, k + 1, K.qTolerance, K.lmBreak, k + 2)) break;      // the q test of THIS iteration: the split step delivers Q directly
                const T bNum = (T)two[0], bDen = (T)sums[0];
                const T betaR = (bDen > T(0)) ? bNum / bDen : T(0);                                 // PCGStep3's guard (solver.t:544-547)
#pragma unroll
                for (int s = 0; s < V; ++s) {      // the restart: p = M r + beta p
                    const long i = (long)s * nT + tid;
                    const Q4<T> d0 = L0[i]; const AoP2<T> d1 = L1[i];
                    V3<T> mo, ma; loadM(s, mo, ma);
                    const V3<T> no{mo.x * rO[s].x + betaR * d0.a, mo.y * rO[s].y + betaR * d0.b, mo.z * rO[s].z + betaR * d0.c};
                    const V3<T> na{ma.x * rA[s].x + betaR * d0.d, ma.y * rA[s].y + betaR * d1.a, ma.z * rA[s].z + betaR * d1.b};
                    L0[i] = Q4<T>{no.x, no.y, no.z, na.x}; L1[i] = AoP2<T>{na.y, na.z};      // (every gather of p_k ended before the barrier of its sums)
                }
                qPending = false; accQ = 0;
                continue;
            }
        }
        // ---- PCGStep2 + PCGStep3 (arap_flatStepPlanes): delta += alpha p, r -= alpha A p, z = M r, p = z + beta p; LM: Q_k = 1/2 sum delta . (r + b) ----
        accQ = 0;
#pragma unroll
        for (int s = 0; s < V; ++s) {
            const long i = (long)s * nT + tid;
            const Q4<T> d0 = L0[i]; const AoP2<T> d1 = L1[i];
            const V3<T> pO{d0.a, d0.b, d0.c}, pA{d0.d, d1.a, d1.b};
            V3<T> mo, ma, bo{0, 0, 0}, ba{0, 0, 0}, dO, dA, pn[2]; loadM(s, mo, ma);
            if constexpr (LMV) loadB(s, bo, ba);
            addToDelta(s, alpha, pO, pA, dO, dA);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const V3<T>&p = h ? pA : pO, &m = h ? ma : mo, &a = h ? aA[s] : aO[s], &d = h ? dA : dO;
                V3<T>& r = h ? rA[s] : rO[s];
                const V3<T> rn{r.x - alpha * a.x, r.y - alpha * a.y, r.z - alpha * a.z};
                const V3<T> z{m.x * rn.x, m.y * rn.y, m.z * rn.z};
                pn[h] = V3<T>{z.x + beta * p.x, z.y + beta * p.y, z.z + beta * p.z};
                if constexpr (LMV) {
                    const V3<T>& bb = h ? ba : bo;
                    if (ok[s]) accQ += (double)(T(0.5) * (d.x * (rn.x + bb.x))) + (double)(T(0.5) * (d.y * (rn.y + bb.y))) + (double)(T(0.5) * (d.z * (rn.z + bb.z)));
                }
                r = rn;
            }
            L0[i] = Q4<T>{pn[0].x, pn[0].y, pn[0].z, pn[1].x}; L1[i] = AoP2<T>{pn[1].y, pn[1].z};      // (every gather of p_k ended before the barrier of its sums)
        }
        qPending = true;
    }
#pragma unroll
    for (int s = 0; s < V; ++s) {      // (a lane reads back what it wrote itself: no barrier)
        const long i = (long)s * nT + tid;
        const Q4<T> e0 = DL0[i]; const AoP2<T> e1 = DL1[i];
        if (ok[s]) { stv3(K.delta, i, V3<T>{e0.a, e0.b, e0.c}); stv3(K.delta + offA, i, V3<T>{e0.d, e1.a, e1.b}); }
    }
}

// ---- host side: which variants are offered (nullptr: not offered).  A variant serves up to V * 512 vertices (LDS: 48 / 96 bytes per vertex).  Every offered kernel holds
// its state in registers without scratch and beats the two-kernel loop at its largest size (profiles/onchip_arap.md).  Not instantiated: V = 4 (2048 vertices: one CU
// takes 14.7 us per iteration where the streaming loop takes 11.9; in double it also spills), and V = 2 in double under Levenberg-Marquardt (spills).
struct AoVariant { int v; const void *gn, *lm; size_t ldsPerVertex; };
template <class T> const std::vector<AoVariant>& aoVariants() {
    static const std::vector<AoVariant> v = [] {
        std::vector<AoVariant> o;
        o.push_back({1, (const void*)arap_onchipPcg<T, 1, false>, (const void*)arap_onchipPcg<T, 1, true>, aoLdsPerVertex<T>()});
        if constexpr (sizeof(T) == 4) o.push_back({2, (const void*)arap_onchipPcg<T, 2, false>, (const void*)arap_onchipPcg<T, 2, true>, aoLdsPerVertex<T>()});
        else o.push_back({2, (const void*)arap_onchipPcg<T, 2, false>, nullptr, aoLdsPerVertex<T>()});
        return o;
    }();
    return v;
}

}  // namespace
}  // namespace optamd
