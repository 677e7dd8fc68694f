// The functor mesh energies (graph_engine.h: cotangent_mesh_smoothing, embedded_mesh_deformation, robust_nonrigid_alignment) on a SMALL mesh: the WHOLE PCG linear
// solve of a Gauss-Newton or Levenberg-Marquardt step as ONE launch of ONE workgroup (solver parameter amd_onchip = 6).  Included by energy_graph_functors.hip behind
// graph_engine.h, so it is compiled with that file's contraction setting (off).  The counterpart of arap_onchip.h for the functor engine, and built like it.
//
// What it replaces: four launches per PCG iteration (PCGStep3, PCGStep1_Graph, PCGStep1, PCGStep2), or two with amd_graph_fused = 1, on meshes of a few hundred vertices,
// where an iteration is launch latency and nothing else.  Here all of the problem sits in one compute unit:
//   p, delta  of every vertex in LDS, in the order of the solver's vectors (unknownIndex): the functors' contexts (EdgeCtx, VertexCtx) read a direction through a pointer,
//             which here points into LDS; delta is there so that the split residual reset can apply A to it;
//   r, A p    of a lane's V vertices in registers (in double, r of cotangent and embedded and A p of cotangent: in LDS beside p and delta, geOcLdsVectors); vertex s * blockDim + tid is slot s of thread tid.  M, b (= r_0)
//             and CtC are re-read from the solver's vectors where they are used: a few kilobytes that stay in the CU's cache;
//   A p       in the record form of the default path.  Edge phase: lanes stride over the hyperedges, each evaluates G::edgeResiduals ONCE with the dual numbers of
//             ge_edges<T, G, 3> and writes one K-scalar record per (slot, hyperedge): into LDS behind the vectors where the host found room (GeOcArgs::recInLds; one flat
//             pointer serves both placements), else into the plan's record buffer (GraphOps::rec, global memory: at head.ply's 4086 four-slot hyperedges the
//             records are 196 KB; the same CU writes and reads them, so the barrier between the phases is all the ordering they need).  Vertex phase: a lane adds its vertex's own residuals (ge_vertices<T, G, 3>'s terms; LM: + CtC p) and the records of the vertex's
//             incidence list, ascending -- one lane per vertex, where ge_vertices folds four: the order of that sum is this kernel's own;
//   sums      the terms of the two-launch loop (graph_pcg.h iterTerm, as ge_gather adds them), formed in double; onchip_sync.h ocWorkgroupSum: the same bits in every lane.
// alpha and beta are ocAlpha / ocBeta (the values of graph_flat_scalars.inc), the update is ge_flatStep's expressions scalar by scalar.  The iterates are those of the
// launch-per-iteration loops up to the order of the sums, which is why the path is opt-in.
// Levenberg-Marquardt as in arap_onchip.h: A = J^T J + diag(CtC), b = r_0, Q carried by the next iteration's sums, the q early-out (ocZetaBreak) reported through
// lmBreak, the split residual reset at every residual_reset_period-th iteration as a second edge + vertex pass over delta.
// Synchronisation: __syncthreads and nothing else.  No polling loop, no co-residency requirement, no time-out path.  Every break is decided from totals that are the same
// bits in every lane, the hyperedge loop runs to a workgroup-uniform trip count with the lanes beyond the last hyperedge masked, and the walk of an incidence list
// contains no barrier: every barrier is reached by every wave.
#pragma once
#include "graph_engine.h"
#include "onchip_sync.h"

namespace optamd {
namespace {

// Which vertices and hyperedges a workgroup works on.  GeOcWhole (ge_onchipPcg): the whole graph -- `vec` (p or delta in LDS) is laid out like the solver's vectors, the
// hyperedges and incidence lists are the graph's own.  GeOcPart (ge_onchipPcgGrid, graph_onchip_grid.h): one part of a partition (graph_partition.h) -- K.g.nE and K.inc
// are the part's, `vec` holds the part's held vertices under local indices, and what the functor reads from memory keeps its global ids.
struct GeOcWhole { static constexpr bool kPart = false; };
template <class G> struct GeOcPart {
    static constexpr bool kPart = true;
    GOff<G> vo;                  // offsets of the unknown images in the part's vectors
    const int* edge;             // global id of the part's hyperedges
    const int* slot[G::V];       // local vertex index of every slot of them
    int nOwn;                    // local indices below this are owned: |J p|^2 of a hyperedge is counted where its slot-0 vertex is
};
template <class T, class G> __device__ __forceinline__ const GOff<G>& geOcVecOffsets(const GeOcArgs<T, G>& K, const GeOcWhole&) { return K.vo; }
template <class T, class G> __device__ __forceinline__ const GOff<G>& geOcVecOffsets(const GeOcArgs<T, G>&, const GeOcPart<G>& loc) { return loc.vo; }
// unknown k of one vertex whose direction sits at index `at` of vec: VertexCtx<T, G, true, true> with the two indices apart
template <class T, class G>
struct GeOcPartVertexCtx {
    typedef Dual<T, 1 + G::K> S;
    const G& g; long v, at; const T* vec; const GOff<G>& vo;
    __device__ __forceinline__ S operator()(int k) const {
        S r(g.X[G::imgOf(k)][v * G::channels(G::imgOf(k)) + G::chOf(k)]);
        r.d[0] = vec[unknownIndex<T, G>(vo, at, k)]; r.d[1 + k] = T(1);
        return r;
    }
};

// How many slots of a hyperedge one evaluation of G::edgeResiduals differentiates: all V -- EdgeCtx's dual, one evaluation per hyperedge and iteration -- unless the functor
// names fewer for a precision (G::kOnChipSlotsPerPass[double]): cotangent's Dual<double, 13> alone takes 216 registers, with the loop state it spilled.  Fewer slots per
// pass mean V / slots evaluations with a shorter dual; forward-mode components do not interact, so the records carry the same bits either way.
template <class T, class G> constexpr int geOcSlotsPerPass() { return G::kOnChipSlotsPerPass[sizeof(T) == 4 ? 0 : 1]; }
// unknown k of vertex j of one hyperedge: component 0 = the direction, components 1 .. NJ K = d/d(unknown k of slot J0 .. J0 + NJ - 1) -- EdgeCtx's seeds of those slots
template <class T, class G, int J0, int NJ>
struct GeOcGroupCtx {
    typedef Dual<T, 1 + NJ * G::K> S;
    const G& g; long vid[G::V]; const T* vec; const GOff<G>& vo;
    __device__ __forceinline__ S operator()(int j, int k) const {
        S r(g.X[G::imgOf(k)][vid[j] * G::channels(G::imgOf(k)) + G::chOf(k)]);
        r.d[0] = vec[unknownIndex<T, G>(vo, vid[j], k)];
        if (j >= J0 && j < J0 + NJ) r.d[1 + (j - J0) * G::K + k] = T(1);
        return r;
    }
};
// ... in a part: the direction of vertex j sits at its local index at[j] of vec (offsets vo: the part's)
template <class T, class G, int J0, int NJ>
struct GeOcPartGroupCtx {
    typedef Dual<T, 1 + NJ * G::K> S;
    const G& g; long vid[G::V]; long at[G::V]; const T* vec; const GOff<G>& vo;
    __device__ __forceinline__ S operator()(int j, int k) const {
        S r(g.X[G::imgOf(k)][vid[j] * G::channels(G::imgOf(k)) + G::chOf(k)]);
        r.d[0] = vec[unknownIndex<T, G>(vo, at[j], k)];
        if (j >= J0 && j < J0 + NJ) r.d[1 + (j - J0) * G::K + k] = T(1);
        return r;
    }
};
// the records of slots J0 .. J0 + NJ - 1 of hyperedge e from residuals whose derivative components 1 .. NJ K belong to those slots: ge_edges<T, G, 3>'s expressions
template <class T, class G, int J0, int NJ, class S>
__device__ __forceinline__ void geOcStoreRecords(const GeOcArgs<T, G>& K, T* rec, const S (&r)[G::RE], long e, bool ok) {
    const int nE = K.g.nE;
#pragma unroll
    for (int j = J0; j < J0 + NJ; ++j) {
#pragma unroll
        for (int k = 0; k < G::K; ++k) {
            T gk = 0;
#pragma unroll
            for (int i = 0; i < G::RE; ++i) {
                if (!G::edgeDepends(i, j, k)) continue;
                gk += r[i].d[1 + (j - J0) * G::K + k] * r[i].d[0];
            }
            if (ok) rec[((long)j * nE + e) * G::K + k] = gk;
        }
    }
}
// (Two bodies, one per view: written as one body over a context type -- or with one context whose index array equals vid[] in the whole-graph view -- the four double
// cotangent ge_onchipPcg kernels allocate other registers (224 .. 248 VGPRs where the build before had 244 .. 256), and their resources are frozen by
// tests/test_onchip_graph_grid_resources.py.  In a part: e is where the records go, eg the hyperedge the functor evaluates, at the local indices of its vertices, cnt whether this workgroup counts its |J vec|^2)
template <class T, class G, bool JP2, int J0, class Loc = GeOcWhole>
__device__ __forceinline__ void geOcSlotGroups(const GeOcArgs<T, G>& K, T* rec, const T* vec, const long (&vid)[G::V], long e, bool ok, double& acc, const Loc& loc = Loc(),
                                               const long* at = nullptr, long eg = 0, bool cnt = false) {
    constexpr int NJ = geOcSlotsPerPass<T, G>();
    static_assert(G::V % NJ == 0, "the slots of a hyperedge divide into whole passes");
    if constexpr (Loc::kPart) {
        typedef GeOcPartGroupCtx<T, G, J0, NJ> Ctx;
        typedef typename Ctx::S S;
        Ctx X{K.g, {}, {}, vec, loc.vo};
#pragma unroll
        for (int j = 0; j < G::V; ++j) { X.vid[j] = vid[j]; X.at[j] = at[j]; }
        S r[G::RE];
        K.g.template edgeResiduals<S>(X, eg, r);
        if (JP2 && J0 == 0 && cnt) { T s = 0; for (int i = 0; i < G::RE; ++i) s += r[i].d[0] * r[i].d[0]; acc += (double)s; }
        geOcStoreRecords<T, G, J0, NJ>(K, rec, r, e, ok);
    } else {
        typedef GeOcGroupCtx<T, G, J0, NJ> Ctx;
        typedef typename Ctx::S S;
        Ctx X{K.g, {}, vec, K.vo};
#pragma unroll
        for (int j = 0; j < G::V; ++j) X.vid[j] = vid[j];
        S r[G::RE];
        K.g.template edgeResiduals<S>(X, e, r);
        if (JP2 && J0 == 0 && ok) { T s = 0; for (int i = 0; i < G::RE; ++i) s += r[i].d[0] * r[i].d[0]; acc += (double)s; }
        geOcStoreRecords<T, G, J0, NJ>(K, rec, r, e, ok);
    }
    if constexpr (J0 + NJ < G::V) geOcSlotGroups<T, G, JP2, J0 + NJ>(K, rec, vec, vid, e, ok, acc, loc, at, eg, cnt);
}

// J^T J vec of every hyperedge as records, rec[(slot * nE + e) * K + k]: ge_edges<T, G, 3> in gather mode, with vec in LDS.  JP2: acc += |J vec|^2, the hyperedges' share
// of vec . A vec (counted once per hyperedge).  Called by every thread of the workgroup.
template <class T, class G, bool JP2, class Loc = GeOcWhole>
__device__ __forceinline__ void geOcEdges(const GeOcArgs<T, G>& K, T* rec, const T* vec, int tid, int nT, double& acc, const Loc& loc = Loc()) {
    const G& g = K.g;
    const int nE = g.nE, nLoop = (nE + nT - 1) / nT * nT;
    for (int e0 = tid; e0 < nLoop; e0 += nT) {
        const bool ok = e0 < nE;
        const long e = ok ? e0 : 0;
        if constexpr (!Loc::kPart && geOcSlotsPerPass<T, G>() == G::V) {
            typedef EdgeCtx<T, G, true, true> Ctx;
            typedef typename Ctx::S S;
            Ctx X{g, {}, vec, K.vo};
#pragma unroll
            for (int j = 0; j < G::V; ++j) X.vid[j] = g.vidx[j][e];
            S r[G::RE];
            g.template edgeResiduals<S>(X, e, r);
            if (JP2 && ok) { T s = 0; for (int i = 0; i < G::RE; ++i) s += r[i].d[0] * r[i].d[0]; acc += (double)s; }
            geOcStoreRecords<T, G, 0, G::V>(K, rec, r, e, ok);
        } else {
            long vid[G::V];
            if constexpr (Loc::kPart) {
                const long eg = loc.edge[e];
                long at[G::V];
#pragma unroll
                for (int j = 0; j < G::V; ++j) { vid[j] = g.vidx[j][eg]; at[j] = loc.slot[j][e]; }
                geOcSlotGroups<T, G, JP2, 0>(K, rec, vec, vid, e, ok, acc, loc, at, eg, ok && at[0] < loc.nOwn);
            } else {
#pragma unroll
                for (int j = 0; j < G::V; ++j) vid[j] = g.vidx[j][e];
                geOcSlotGroups<T, G, JP2, 0>(K, rec, vec, vid, e, ok, acc);
            }
        }
    }
}

// (J^T J vec)(v) [+ CtC vec] of vertex v: its own residuals' part, then the records of its (hyperedge, slot) pairs in ascending order, four loads in flight.
// acc += vec(v) . (own part).  A lane without a vertex (ok == false) evaluates vertex 0 and adds nothing.  In a part (GeOcPart) v is the vertex's global id and `at` its
// local index: the position of its direction in vec and of its list in K.inc.
template <class T, class G, bool LMV, class Loc = GeOcWhole>
__device__ __forceinline__ void geOcVertex(const GeOcArgs<T, G>& K, const T* rec, const T* vec, long v, bool ok, T (&gs)[G::K], double& acc, const Loc& loc = Loc(), long at = 0) {
    constexpr int BATCH = 4;
    const long vv = ok ? v : 0;
    const long va = Loc::kPart ? (ok ? at : 0) : vv;
    const GOff<G>& vvo = geOcVecOffsets<T, G>(K, loc);
    typedef VertexCtx<T, G, true, true> Ctx;
    typedef typename Ctx::S S;
    S r[G::RV > 0 ? G::RV : 1];
    if constexpr (Loc::kPart) K.g.template vertexResiduals<S>(GeOcPartVertexCtx<T, G>{K.g, vv, va, vec, vvo}, vv, r);
    else K.g.template vertexResiduals<S>(Ctx{K.g, vv, vec, K.vo}, vv, r);
#pragma unroll
    for (int k = 0; k < G::K; ++k) {
        T gk = 0;
#pragma unroll
        for (int i = 0; i < G::RV; ++i) gk += r[i].d[1 + k] * r[i].d[0];
        const long u = unknownIndex<T, G>(K.vo, vv, k), uv = unknownIndex<T, G>(vvo, va, k);
        if (LMV) gk += K.CtC[u] * vec[uv];
        if (ok) acc += (double)(vec[uv] * gk);
        gs[k] = gk;
    }
    const int tb = ok ? K.inc.off[va] : 0, te = ok ? K.inc.off[va + 1] : 0;
    for (int t0 = tb; t0 < te; t0 += BATCH) {
        int id[BATCH]; T q[BATCH][G::K];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) id[b] = K.inc.idx[min(t0 + b, te - 1)];
#pragma unroll
        for (int b = 0; b < BATCH; ++b)
#pragma unroll
            for (int k = 0; k < G::K; ++k) q[b][k] = rec[(long)id[b] * G::K + k];
#pragma unroll
        for (int b = 0; b < BATCH; ++b)
            if (t0 + b < te) {
#pragma unroll
                for (int k = 0; k < G::K; ++k) gs[k] += q[b][k];
            }
    }
}

template <class T, class G, int V, bool LMV>
__global__ __launch_bounds__(kOcWgMaxBlock) void ge_onchipPcg(GeOcArgs<T, G> K) {
    constexpr int NS = LMV ? 5 : 4, NK = G::K;
    extern __shared__ __align__(16) unsigned char geOcLds[];
    __shared__ __align__(16) double red[NS * kOcWgMaxWaves];
    __shared__ __align__(16) double red2[2 * kOcWgMaxWaves];
    const int tid = threadIdx.x, nT = blockDim.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), nW = nT >> 6;
    const long N = K.g.N;
    // p and delta of every vertex in the order of the solver's vectors: a lane writes its own vertices' entries, the edge phase reads everybody's
    // (and r, where the functor says so: the dual numbers of a double hyperedge leave no registers for it)
    constexpr bool RREG = geOcLdsVectors<T, G>() == 2;
    T* const PL = reinterpret_cast<T*>(geOcLds); T* const DL = PL + K.nScalars; T* const RL = DL + K.nScalars;
    // the records of this iteration: in LDS behind the vectors where the host found room for them (one pointer for both placements: a flat address), else the plan's buffer
    T* const REC = K.recInLds ? PL + (long)geOcLdsVectors<T, G>() * K.nScalars : K.rec;
    for (int e = tid; e < NS * kOcWgMaxWaves; e += nT) red[e] = 0.0;
    for (int e = tid; e < 2 * kOcWgMaxWaves; e += nT) red2[e] = 0.0;

    constexpr bool AREG = geOcLdsVectors<T, G>() < 4;      // (4: A p in LDS as well)
    T* const AL = RL + K.nScalars;
    T r[RREG ? V : 1][RREG ? NK : 1], ap[AREG ? V : 1][AREG ? NK : 1];
    auto getAp = [&](int s, int c, long u) { return AREG ? ap[AREG ? s : 0][AREG ? c : 0] : AL[u]; };
    auto setAp = [&](int s, int c, long u, T x) { if (AREG) ap[AREG ? s : 0][AREG ? c : 0] = x; else AL[u] = x; };
    bool ok[V];
    auto getR = [&](int s, int c, long u) { return RREG ? r[RREG ? s : 0][RREG ? c : 0] : RL[u]; };
    auto setR = [&](int s, int c, long u, T x) { if (RREG) r[RREG ? s : 0][RREG ? c : 0] = x; else RL[u] = x; };
#pragma unroll
    for (int s = 0; s < V; ++s) {
        const long v = (long)s * nT + tid;
        ok[s] = v < N;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            const long u = unknownIndex<T, G>(K.vo, ok[s] ? v : 0, c);
            if (AREG) setAp(s, c, u, T(0));
            if (ok[s]) { PL[u] = K.p0[u]; DL[u] = T(0); setR(s, c, u, K.r0[u]); }
            else if (RREG) setR(s, c, u, T(0));
        }
    }
    // delta += alpha p of slot s (PCGStep2's first half, solver.t:461-462)
    auto addToDelta = [&](int s, T alpha) {
        if (!ok[s]) return;
        const long v = (long)s * nT + tid;
#pragma unroll
        for (int c = 0; c < NK; ++c) { const long u = unknownIndex<T, G>(K.vo, v, c); DL[u] = DL[u] + alpha * PL[u]; }
    };

    double accQ = 0;
    T Q0 = 0;                 // fetchQ before the loop (solver.t:1050): delta = 0, so exactly 0
    bool qPending = false;    // LM: the Q of the iteration before travels with this iteration's sums
    for (int k = 0; k < K.L; ++k) {
        __syncthreads();      // every vertex's p is in LDS; every read of the records of the pass before has ended
        // ---- PCGStep1_Graph + PCGStep1: A p_k with the sums of the expanded beta numerator ----
        double sums[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) sums[q] = 0;
        geOcEdges<T, G, true>(K, REC, PL, tid, nT, sums[1]);
        __syncthreads();      // every record of p_k is written
#pragma unroll
        for (int s = 0; s < V; ++s) {
            const long v = (long)s * nT + tid;
            T avl[NK];      // (A p of this slot: the lane's registers, or a local on its way to LDS)
            auto& av = [&]() -> T(&)[NK] { if constexpr (AREG) return ap[s]; else return avl; }();
            geOcVertex<T, G, LMV>(K, REC, PL, v, ok[s], av, sums[1]);
            if (ok[s]) {
#pragma unroll
                for (int c = 0; c < NK; ++c) {
                    const long u = unknownIndex<T, G>(K.vo, v, c);
                    const T m = K.M[u], rr = getR(s, c, u), a = av[c];
                    sums[0] += iterTerm(m, rr, rr); sums[2] += iterTerm(m, rr, a); sums[3] += iterTerm(m, a, a);
                    if (!AREG) setAp(s, c, u, a);
                }
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
            for (int s = 0; s < V; ++s) addToDelta(s, alpha);
            if (last) break;
        }
        if constexpr (LMV) {
            if (K.resetPeriod > 0 && (k + 1) % K.resetPeriod == 0) {
                // ---- the split residual reset (solver.t:1077-1083) behind delta += alpha p: r = b - (J^T J + CtC) delta; z = M r; sum r . z and Q directly ----
                __syncthreads();      // every vertex's delta is in LDS (and every read of the records of p_k ended before the barrier of the sums)
                double two[2] = {0, 0}, unused = 0;
                geOcEdges<T, G, false>(K, REC, DL, tid, nT, unused);
                __syncthreads();      // every record of delta is written
#pragma unroll
                for (int s = 0; s < V; ++s) {
                    const long v = (long)s * nT + tid;
                    T ad[NK];
                    geOcVertex<T, G, LMV>(K, REC, DL, v, ok[s], ad, unused);
                    if (ok[s]) {      // k_step2SecondHalf's sums, scalar by scalar
#pragma unroll
                        for (int c = 0; c < NK; ++c) {
                            const long u = unknownIndex<T, G>(K.vo, v, c);
                            const T bb = K.r0[u], mm = K.M[u], dd = DL[u], rr = bb - ad[c];
                            setR(s, c, u, rr);
                            const T zz = mm * rr;
                            two[0] += (double)(zz * rr); two[1] += (double)(T(0.5) * (dd * (rr + bb)));
                        }
                    }
                }
                ocWorkgroupSum<2>(two, red2, lane, wave, nW);
                if (ocZetaBreak((T)two[1], Q0, k + 1, K.qTolerance, K.lmBreak, k + 2)) break;      // the q test of THIS iteration: the split step delivers Q directly
                const T bNum = (T)two[0], bDen = (T)sums[0];
                const T betaR = (bDen > T(0)) ? bNum / bDen : T(0);                                 // PCGStep3's guard (solver.t:544-547)
#pragma unroll
                for (int s = 0; s < V; ++s) {      // the restart: p = M r + beta p  (every read of p_k by another lane ended before the barrier of the sums)
                    const long v = (long)s * nT + tid;
                    if (!ok[s]) continue;
#pragma unroll
                    for (int c = 0; c < NK; ++c) { const long u = unknownIndex<T, G>(K.vo, v, c); PL[u] = K.M[u] * getR(s, c, u) + betaR * PL[u]; }
                }
                qPending = false; accQ = 0;
                continue;
            }
        }
        // ---- PCGStep2 + PCGStep3 (ge_flatStep's expressions): delta += alpha p, r -= alpha A p, z = M r, p = z + beta p; LM: Q_k = 1/2 sum delta . (r + b) ----
        accQ = 0;
#pragma unroll
        for (int s = 0; s < V; ++s) {
            const long v = (long)s * nT + tid;
            if (!ok[s]) continue;
#pragma unroll
            for (int c = 0; c < NK; ++c) {
                const long u = unknownIndex<T, G>(K.vo, v, c);
                const T p = PL[u], m = K.M[u];
                const T d = DL[u] + alpha * p;
                const T rn = getR(s, c, u) - alpha * getAp(s, c, u);
                const T z = m * rn;
                const T pn = z + beta * p;
                if constexpr (LMV) accQ += (double)(T(0.5) * (d * (rn + K.r0[u])));      // b = r_0 (solver.t:657)
                DL[u] = d; setR(s, c, u, rn); PL[u] = pn;      // (every read of p_k by another lane ended before the barrier of the sums)
            }
        }
        qPending = true;
    }
#pragma unroll
    for (int s = 0; s < V; ++s) {      // (a lane reads back what it wrote itself: no barrier)
        const long v = (long)s * nT + tid;
        if (!ok[s]) continue;
#pragma unroll
        for (int c = 0; c < NK; ++c) { const long u = unknownIndex<T, G>(K.vo, v, c); K.delta[u] = DL[u]; }
    }
}

// ---- host side: which variants are offered.  A variant serves up to V * 512 vertices; p and delta (and r, and A p: G::kOnChipLdsVectors) take 2 K (3 K, 4 K) scalars of LDS per vertex.  The functor says up to which V
// it is offered per (precision, solver): G::kOnChipV[double][LM], 0 = none -- a variant that would spill, or whose largest mesh does not fit LDS (embedded in double at
// V = 2: 196 KB), is not instantiated.  GraphOps filters the list once more at first use by what the device reports (graph_engine.h ocInit).
template <class T, class G, int V>
void geOcOffer(std::vector<GeOcVariant>& o) {
    constexpr int P = sizeof(T) == 4 ? 0 : 1;
    const void *gn = nullptr, *lm = nullptr;
    if constexpr (G::kOnChipV[P][0] >= V) gn = (const void*)ge_onchipPcg<T, G, V, false>;
    if constexpr (G::kOnChipV[P][1] >= V) lm = (const void*)ge_onchipPcg<T, G, V, true>;
    if (gn || lm) o.push_back({V, gn, lm});
}
template <class T, class G> const std::vector<GeOcVariant>& geOcVariants() {
    static const std::vector<GeOcVariant> v = [] {
        std::vector<GeOcVariant> o;
        geOcOffer<T, G, 1>(o); geOcOffer<T, G, 2>(o);
        return o;
    }();
    return v;
}

}  // namespace
}  // namespace optamd
