// The functor mesh energies on a mesh too large (or too much arithmetic) for one workgroup: the WHOLE PCG linear solve of a Gauss-Newton or Levenberg-Marquardt step as
// ONE persistent launch of G > 1 workgroups (solver parameter amd_onchip = 7; amd_onchip_workgroups).  Included by energy_graph_functors.hip behind graph_onchip.h, so it
// is compiled with that file's contraction setting (off).  The phases are ge_onchipPcg's (graph_onchip.h: geOcEdges, geOcVertex, ocAlpha, ocBeta, ocZetaBreak, the update's
// expressions), the protocol between the workgroups is the image kernels' (stencil_onchip.h; onchip_sync.h ocGridSum).
//
// Partition (graph_partition.h, built on the host with the incidence lists): a workgroup OWNS a connected chunk of the vertices, evaluates every hyperedge that touches one
// of them (a cut hyperedge is evaluated by each side: records never cross workgroups) and HOLDS p, delta, r and A p of every vertex of those hyperedges in LDS, under local
// indices: owned vertices first, then the halo.
// One grid-wide wait per PCG iteration (one more per split residual reset):
//   edge phase over the workgroup's hyperedges; barrier; vertex phase over its owned vertices, where A p of an owned vertex that is halo elsewhere goes out as tagged words
//   (its wire) BEFORE the sums are posted; ocGridSum with the halo's A p as its ring.  Behind the wait owner and halo holders apply r -= alpha A p; p = M r + beta p;
//   delta += alpha p with the same alpha and beta and the same expressions: the same bits, so p itself never travels.
// Everything that crosses workgroups is a {payload, tag} word written by ocStore and read by ocLoad (relaxed, agent scope); tags count phases, buffers alternate by the
// tag's parity.  No plain load reads another workgroup's data; r_0, p_0, M, CtC and the partition's lists were written by earlier kernels of the stream and are read plainly.
// A workgroup's records stay its own (LDS, or its slab of GraphOps::ggRec).
// Every wait is bounded (the first by OcTimeouts::first: passing it proves the grid resident before anything is written); a wait that gives up raises `bad`, every
// workgroup then leaves its loop at its next sum, and ocApplyDelta (Gauss-Newton) or this kernel (Levenberg-Marquardt) tells the host.  The hyperedge and vertex loops run
// to workgroup-uniform trip counts with masked lanes and every break is decided from totals that are the same bits everywhere: every barrier is reached by every wave.
// Sums: ge_onchipPcg's terms, formed over owned vertices only, |J p|^2 once per hyperedge (by the owner of its slot-0 vertex); every workgroup adds all workgroups' words in
// workgroup order.  A vertex's A p is its own part plus its records in ascending global id -- ge_onchipPcg's order, so A p has the same bits for every G.
#pragma once
#include "graph_onchip.h"

namespace optamd {
namespace {

template <class T, class G, bool LMV>
__global__ __launch_bounds__(kOcWgMaxBlock) void ge_onchipPcgGrid(GeGridArgs<T, G> A) {
    constexpr int NS = LMV ? 5 : 4, NK = G::K, NWD = sizeof(T) / 4, RING = kGeGridRing;
    extern __shared__ __align__(16) unsigned char geGridLds[];
    __shared__ OcSumLds<NS, kOcWgMaxWaves, kGeGridSumG> S;
    const int tid = threadIdx.x, nT = kOcWgMaxBlock, wg = blockIdx.x;
    const GeGridPart D = A.parts[wg];
    const int nOwn = D.nOwn, nS = D.nHeld * NK;
    const int* const held = A.lists + D.oHeld; const int* const wire = A.lists + D.oWire; const int* const gidx = A.lists + D.oGidx; const int* const recv = A.lists + D.oRecv;
    // the part as geOcEdges / geOcVertex see it: its hyperedge count and incidence lists in K, the local indices in loc
    GeOcArgs<T, G> K = A.k;
    K.g.nE = D.nE; K.inc = Incidence{A.lists + D.oIncOff, A.lists + D.oIncIdx};
    GeOcPart<G> loc;
    { long o = 0; for (int i = 0; i < G::NIMG; ++i) { loc.vo.o[i] = o; o += (long)D.nHeld * G::channels(i); } }
    loc.edge = A.lists + D.oEdge; loc.nOwn = nOwn;
#pragma unroll
    for (int j = 0; j < G::V; ++j) loc.slot[j] = A.lists + D.oSlot + (long)j * D.nE;
    // p, delta, r, A p of the held vertices; behind them this iteration's records where every workgroup's fit (else: the workgroup's slab of the partition's record buffer)
    T* const PL = reinterpret_cast<T*>(geGridLds); T* const DL = PL + nS; T* const RL = DL + nS; T* const AL = RL + nS;
    T* const REC = A.k.recInLds ? AL + nS : A.k.rec + (long)D.recBase * NK;
    for (int u = tid; u < nS; u += nT) { const int gi = gidx[u] & 0x7fffffff; PL[u] = A.k.p0[gi]; DL[u] = T(0); RL[u] = A.k.r0[gi]; AL[u] = T(0); }
    // the ring: A p of the halo, scalar h of it under box index recv[2 h], for the held scalar recv[2 h + 1]; lane tid asks for scalars tid, tid + 512, ...
    int rb[RING], ru[RING];
#pragma unroll
    for (int q = 0; q < RING; ++q) { const int h = tid + q * nT; const bool has = h < D.nRecv; rb[q] = has ? recv[2 * h] : -1; ru[q] = has ? recv[2 * h + 1] : 0; }
    oc_u64 rw[RING][NWD];
    const int nOwnLoop = (nOwn + nT - 1) / nT * nT;
    unsigned ph = 0;      // phases passed: tag = tag0 + ph
    bool failed = false;

    // the grid-wide sum of one phase with the halo's A vec as its ring; afterwards AL holds A vec of every held vertex.  false: a wait gave up
    auto sumAndCollect = [&](const double (&part)[NS]) {
        const unsigned tag = A.tag0 + ph;
        oc_u64* const slotPar = A.slots + (size_t)(tag & 1u) * kGeGridSumG * 2 * NS;
        const oc_u64* const boxPar = A.box + (size_t)(tag & 1u) * A.boxWords;
        auto askRing = [&]() {
#pragma unroll
            for (int q = 0; q < RING; ++q)
#pragma unroll
                for (int d = 0; d < NWD; ++d) rw[q][d] = rb[q] >= 0 ? ocLoad(boxPar + (size_t)rb[q] * NWD + d) : ((oc_u64)tag << 32);
        };
        auto ringHere = [&]() {
            bool ok = true;
#pragma unroll
            for (int q = 0; q < RING; ++q)
#pragma unroll
                for (int d = 0; d < NWD; ++d) ok = ok && (unsigned)(rw[q][d] >> 32) == tag;
            return ok;
        };
        ocGridSum(S, part, tag, slotPar, A.nG, A.bad, ph == 0 ? A.firstTicks : A.laterTicks, askRing, ringHere);
        ++ph;
        if (S.gaveUp) return false;
#pragma unroll
        for (int q = 0; q < RING; ++q) if (rb[q] >= 0) AL[ru[q]] = ocPayload<T>(rw[q]);
        __syncthreads();      // A vec of the halo is in LDS
        return true;
    };
    // A vec of the owned vertices (geOcVertex; LM: + CtC vec) into AL and onto the wires; per scalar f(local index, global index, A vec) for the caller's sums
    auto vertexPhase = [&](const T* vec, double& dot, auto&& f) {
        const unsigned tag = A.tag0 + ph;
        oc_u64* const boxPar = A.box + (size_t)(tag & 1u) * A.boxWords;
        for (int i0 = tid; i0 < nOwnLoop; i0 += nT) {
            const bool ok = i0 < nOwn;
            const int i = ok ? i0 : 0;
            const long v = held[i];
            T av[NK];
            geOcVertex<T, G, LMV>(K, REC, vec, v, ok, av, dot, loc, i);
            if (!ok) continue;      // (no barrier below)
            const int w = wire[i];
#pragma unroll
            for (int c = 0; c < NK; ++c) {
                const long ul = unknownIndex<T, G>(loc.vo, i, c), ug = unknownIndex<T, G>(A.k.vo, v, c);
                AL[ul] = av[c];
                if (w >= 0) ocSend(boxPar, w * NK + c, av[c], tag);
                f(ul, ug, av[c]);
            }
        }
    };

    double accQ = 0;
    T Q0 = 0;                 // fetchQ before the loop (solver.t:1050): delta = 0, so exactly 0
    bool qPending = false;    // LM: the Q of the iteration before travels with this iteration's sums
    for (int k = 0; k < A.k.L; ++k) {
        if (k == A.failAt && wg == 0 && tid == 0) __hip_atomic_store(A.bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (test hook: as a timed-out wait would)
        __syncthreads();      // every held vertex's p is in LDS; every read of the records of the pass before has ended
        double sums[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) sums[q] = 0;
        geOcEdges<T, G, true>(K, REC, PL, tid, nT, sums[1], loc);
        __syncthreads();      // every record of p_k is written
        vertexPhase(PL, sums[1], [&](long ul, long ug, T a) {
            const T m = A.k.M[ug], rr = RL[ul];
            sums[0] += iterTerm(m, rr, rr); sums[2] += iterTerm(m, rr, a); sums[3] += iterTerm(m, a, a);
        });
        if constexpr (LMV) sums[NS - 1] = accQ;
        if (!sumAndCollect(sums)) { failed = true; break; }
        double tot[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) tot[q] = S.TOT[q];
        if (A.k.trace && wg == 0 && tid == 0) { A.k.trace[4 * k] = tot[0]; A.k.trace[4 * k + 1] = tot[1]; A.k.trace[4 * k + 2] = tot[2]; A.k.trace[4 * k + 3] = tot[3]; }
        if constexpr (LMV) {      // the q early-out of iteration k - 1 (solver.t:1093-1102): nothing of iteration k has been applied yet
            if (qPending && ocZetaBreak((T)tot[NS - 1], Q0, k, A.k.qTolerance, A.k.lmBreak, k + 1)) break;
        }
        const T alpha = ocAlpha<T>(tot[0], tot[1]);
        const T beta = ocBeta<T>(alpha, tot[0], tot[2], tot[3], tot[0]);
        const bool last = k + 1 == A.k.L;      // after the last iteration only delta survives
        const bool reset = LMV && A.k.resetPeriod > 0 && (k + 1) % A.k.resetPeriod == 0;
        if (last || reset) {
            for (int u = tid; u < nS; u += nT) DL[u] = DL[u] + alpha * PL[u];      // delta += alpha p (PCGStep2's first half)
            if (last) break;
        }
        if constexpr (LMV) {
            if (reset) {
                // ---- the split residual reset (solver.t:1077-1083) behind delta += alpha p: r = b - (J^T J + CtC) delta; z = M r; sum r . z and Q directly ----
                __syncthreads();      // every held vertex's delta is in LDS
                double two[NS], unused = 0;
#pragma unroll
                for (int q = 0; q < NS; ++q) two[q] = 0;
                geOcEdges<T, G, false>(K, REC, DL, tid, nT, unused, loc);
                __syncthreads();      // every record of delta is written
                vertexPhase(DL, unused, [&](long ul, long ug, T ad) {      // k_step2SecondHalf's sums, scalar by scalar
                    const T bb = A.k.r0[ug], mm = A.k.M[ug], dd = DL[ul], rr = bb - ad;
                    const T zz = mm * rr;
                    two[0] += (double)(zz * rr); two[1] += (double)(T(0.5) * (dd * (rr + bb)));
                });
                if (!sumAndCollect(two)) { failed = true; break; }
                const double t0 = S.TOT[0], t1 = S.TOT[1];
                if (ocZetaBreak((T)t1, Q0, k + 1, A.k.qTolerance, A.k.lmBreak, k + 2)) break;      // the q test of THIS iteration: the split step delivers Q directly
                const T bNum = (T)t0, bDen = (T)tot[0];
                const T betaR = (bDen > T(0)) ? bNum / bDen : T(0);                               // PCGStep3's guard (solver.t:544-547)
                for (int u = tid; u < nS; u += nT) {      // r = b - A delta and the restart p = M r + beta p, on owned and halo alike
                    const int gi = gidx[u] & 0x7fffffff;
                    const T rr = A.k.r0[gi] - AL[u];
                    RL[u] = rr; PL[u] = A.k.M[gi] * rr + betaR * PL[u];
                }
                qPending = false; accQ = 0;
                continue;
            }
        }
        // ---- PCGStep2 + PCGStep3 (ge_flatStep's expressions) on owned and halo alike; LM: Q_k = 1/2 sum delta . (r + b) over the owned ----
        accQ = 0;
        for (int u = tid; u < nS; u += nT) {
            const int gw = gidx[u], gi = gw & 0x7fffffff;
            const T p = PL[u], m = A.k.M[gi];
            const T d = DL[u] + alpha * p;
            const T rn = RL[u] - alpha * AL[u];
            const T z = m * rn;
            const T pn = z + beta * p;
            if constexpr (LMV) { if (gw >= 0) accQ += (double)(T(0.5) * (d * (rn + A.k.r0[gi]))); }      // b = r_0 (solver.t:657)
            DL[u] = d; RL[u] = rn; PL[u] = pn;      // (every read of p_k by another lane ended before the barriers of the sums)
        }
        qPending = true;
    }
    if (failed) {      // a wait gave up: delta is not written; LM: the solver applies the update itself and is told here
        if (tid == 0 && A.hostErr) __hip_atomic_store(A.hostErr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    __syncthreads();      // (the last delta += alpha p was written by other lanes)
    for (int u = tid; u < nS; u += nT) { const int gw = gidx[u]; if (gw >= 0) A.k.delta[gw] = DL[u]; }
}

// ---- host side: the kernels of a functor and precision, [Gauss-Newton, Levenberg-Marquardt] ----
template <class T, class G> GeGridKernels geGridKernels() { return GeGridKernels{(const void*)ge_onchipPcgGrid<T, G, false>, (const void*)ge_onchipPcgGrid<T, G, true>}; }

}  // namespace
}  // namespace optamd
