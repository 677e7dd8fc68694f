// Functor-driven kernel set for energies on meshes: residuals per vertex plus residuals per hyperedge of a graph.
//
// Counterpart of stencil_engine.h for the graph domain (reference o.t:2092-2126 applyJTJ_Graph, :2228-2253 evalJTF_Graph;
// solverGPUGaussNewton.t:687-706).  The energy is a device functor that writes its vertex residuals and its edge residuals once
// against a scalar type S; the engine instantiates them with plain and dual numbers:
//   edge pass (one thread per hyperedge): S = Dual<T, V*K (+1)> over the V vertices of the edge; its J^T (J p) contributions go into one
//                K-scalar record per (hyperedge, slot),
//   vertex pass (one thread per vertex): the contribution of the vertex's own residuals (+ CtC p) plus the records of every (hyperedge, slot)
//                the vertex occupies, in ascending (slot, hyperedge) order from incidence lists built once per graph by a counting sort (graph_lists.h VertexLists).
// No atomics: unlike the reference's graph kernels (one atomic per (vertex, unknown), unordered) a solve is bit-reproducible.
// OPT_AMD_GRAPH_GATHER=0 selects the scatter formulation instead (wave-aggregated atomics for the first vertex, whose edges arrive
// grouped, OptGraph.h:64-76; plain atomics for the others).
// Solver parameter amd_graph_fused = 1: J^T J p as ONE launch that evaluates every record in place (ge_gather: the same bits) and the PCG iteration as two launches
// (ge_flatStep + ge_gather) through the solver's launch-per-iteration loops, where the default runs the reference's sequence in four.
// Solver parameter amd_onchip = 6: on a mesh small enough for one workgroup the WHOLE linear solve is one launch (graph_onchip.h ge_onchipPcg; GraphOps::pcgSolveOnChip).
// Solver parameter amd_onchip = 7: ... or one persistent launch of several workgroups over a partition of the mesh (graph_onchip_grid.h ge_onchipPcgGrid; GraphOps::gg*).
// The functor G provides (constexpr / static): NIMG, K, imgOf(k), chOf(k), channels(img), V, RV, RE, edgeDepends(ri, j, k), kName (for OptAmd_PlanDescribe), kSlotAtRunTime (ge_slotDispatch), kOnChipV, kOnChipSlotsPerPass, kOnChipLdsVectors (graph_onchip.h);
// members N, nE, vidx[V], X[NIMG]; host bindParams(void**), unknownParam(img).
#pragma once
#include "stencil_engine.h"
#include "graph_pcg.h"
#include "onchip_sync.h"
#include "graph_partition.h"
#include "graph_lists.h"      // VertexLists: the incidence lists, built once per graph

namespace optamd {

template <class G> struct GOff { long o[G::NIMG]; };

template <class T, class G> __device__ __forceinline__ long unknownIndex(const GOff<G>& vo, long vertex, int k) {
    return vo.o[G::imgOf(k)] + vertex * G::channels(G::imgOf(k)) + G::chOf(k);
}
// unknown k of one vertex.  DIR: slot 0 = component of the solver vector `vec`; SEED: slots DIR.. = d/d(unknown k)
template <class T, class G, bool DIR, bool SEED>
struct VertexCtx {
    static constexpr int N = (DIR ? 1 : 0) + (SEED ? G::K : 0);
    typedef typename std::conditional<N == 0, T, Dual<T, (N > 0 ? N : 1)>>::type S;
    const G& g; long v; const T* vec; const GOff<G>& vo;
    __device__ __forceinline__ S operator()(int k) const {
        const T x = g.X[G::imgOf(k)][v * G::channels(G::imgOf(k)) + G::chOf(k)];
        if constexpr (N == 0) return x;
        else { S r(x); if (DIR) r.d[0] = vec[unknownIndex<T, G>(vo, v, k)]; if (SEED) r.d[(DIR ? 1 : 0) + k] = T(1); return r; }
    }
};
// unknown k of vertex j of one hyperedge
template <class T, class G, bool DIR, bool SEED>
struct EdgeCtx {
    static constexpr int N = (DIR ? 1 : 0) + (SEED ? G::V * G::K : 0);
    typedef typename std::conditional<N == 0, T, Dual<T, (N > 0 ? N : 1)>>::type S;
    const G& g; long vid[G::V]; const T* vec; const GOff<G>& vo;
    __device__ __forceinline__ S operator()(int j, int k) const {
        const T x = g.X[G::imgOf(k)][vid[j] * G::channels(G::imgOf(k)) + G::chOf(k)];
        if constexpr (N == 0) return x;
        else { S r(x); if (DIR) r.d[0] = vec[unknownIndex<T, G>(vo, vid[j], k)]; if (SEED) r.d[(DIR ? 1 : 0) + j * G::K + k] = T(1); return r; }
    }
};

// ---- incidence lists: for every vertex the ids j * nE + e of the (hyperedge e, slot j) pairs it occupies, ascending (graph_lists.h VertexLists) ----
struct Incidence { const int* off; const int* idx; };       // off == nullptr: scatter mode

// MODE 0: cost, 1: model cost (vec = delta), 2: J^T F + diag, 3: J^T J vec.  LANES > 1 (gather mode): LANES adjacent lanes share one vertex;
// lane 0 evaluates the vertex's own residuals, every lane walks every LANES-th record of the incidence list, and the partial sums are
// folded with shuffles in a fixed order (more independent loads in flight than one thread walking ~24 records).
#ifndef GE_GATHER_LANES
#define GE_GATHER_LANES 4
#endif
template <class T, class G, int MODE, int LANES = 1>
__global__ __launch_bounds__(kBlock) void ge_vertices(G g, const T* __restrict__ vec, GOff<G> vo, T* __restrict__ out, T* __restrict__ diag, const T* __restrict__ CtC,
                                                       double* __restrict__ partials, Incidence inc = Incidence{nullptr, nullptr}, const T* __restrict__ rec = nullptr) {
    __shared__ double scratch[kBlock / kWave + 1];
    double acc = 0;
    const int sub = LANES > 1 ? threadIdx.x % LANES : 0;
    for (long v = (blockIdx.x * (long)blockDim.x + threadIdx.x) / LANES; v < g.N; v += (long)gridDim.x * blockDim.x / LANES) {
        typedef VertexCtx<T, G, MODE == 1 || MODE == 3, MODE >= 2> Ctx;
        typedef typename Ctx::S S;
        S r[G::RV > 0 ? G::RV : 1];
        if (sub == 0) g.template vertexResiduals<S>(Ctx{g, v, vec, vo}, v, r);
        if constexpr (MODE == 0) { T s = 0; for (int i = 0; i < G::RV; ++i) s += r[i] * r[i]; acc += (double)(T(0.5) * s); }
        else if constexpr (MODE == 1) { T s = 0; for (int i = 0; i < G::RV; ++i) { const T m = r[i].v + r[i].d[0]; s += m * m; } acc += (double)(T(0.5) * s); }
        else {
            T gs[G::K], ds[G::K];
#pragma unroll
            for (int k = 0; k < G::K; ++k) {
                T gk = 0, dk = 0;
                if (sub == 0) {
#pragma unroll
                    for (int i = 0; i < G::RV; ++i) {
                        if (MODE == 2) { gk += r[i].d[k] * r[i].v; dk += r[i].d[k] * r[i].d[k]; }
                        else gk += r[i].d[1 + k] * r[i].d[0];
                    }
                    if (MODE == 3) { const long u = unknownIndex<T, G>(vo, v, k); if (CtC) gk += CtC[u] * vec[u]; acc += (double)(vec[u] * gk); }   // the edges' share of p . A p is |J p|^2, summed by the edge pass
                }
                gs[k] = gk; ds[k] = dk;
            }
            if (inc.off) {      // gather mode: add the records of the (hyperedge, slot) pairs of this vertex, ascending
                constexpr int KK = MODE == 2 ? 2 * G::K : G::K;
                for (int t = inc.off[v] + sub, te = inc.off[v + 1]; t < te; t += LANES) {
                    const T* q = rec + (long)inc.idx[t] * KK;
#pragma unroll
                    for (int k = 0; k < G::K; ++k) { gs[k] += q[k]; if (MODE == 2) ds[k] += q[G::K + k]; }
                }
                if (LANES > 1) {
#pragma unroll
                    for (int off = LANES / 2; off > 0; off >>= 1)
#pragma unroll
                        for (int k = 0; k < G::K; ++k) { gs[k] += __shfl_down(gs[k], off, LANES); if (MODE == 2) ds[k] += __shfl_down(ds[k], off, LANES); }
                }
            }
            if (sub == 0) {
#pragma unroll
                for (int k = 0; k < G::K; ++k) {
                    const long u = unknownIndex<T, G>(vo, v, k);
                    if (MODE == 2) { out[u] = -gs[k]; diag[u] = ds[k]; } else out[u] = gs[k];
                }
            }
        }
    }
    if (MODE != 2) { const double t = blockReduceSum(acc, scratch); if (threadIdx.x == 0 && partials) partials[blockIdx.x] = t; }
}

template <class T, class G, int MODE>
__global__ __launch_bounds__(kBlock) void ge_edges(G g, const T* __restrict__ vec, GOff<G> vo, T* __restrict__ out, T* __restrict__ diag, double* __restrict__ partials,
                                                    T* __restrict__ rec = nullptr) {
    __shared__ double scratch[kBlock / kWave + 1];
    double acc = 0;
    const long nE = g.nE, nLoop = ((nE + kBlock - 1) / kBlock) * kBlock;       // whole waves stay in the loop: the aggregation shuffles need them
    for (long e0 = blockIdx.x * (long)blockDim.x + threadIdx.x; e0 < nLoop; e0 += (long)gridDim.x * blockDim.x) {
        const bool ok = e0 < nE;
        const long e = ok ? e0 : 0;
        typedef EdgeCtx<T, G, MODE == 1 || MODE == 3, MODE >= 2> Ctx;
        typedef typename Ctx::S S;
        Ctx X{g, {}, vec, vo};
#pragma unroll
        for (int j = 0; j < G::V; ++j) X.vid[j] = g.vidx[j][e];
        S r[G::RE];
        g.template edgeResiduals<S>(X, e, r);
        if constexpr (MODE == 0) { T s = 0; for (int i = 0; i < G::RE; ++i) s += r[i] * r[i]; if (ok) acc += (double)(T(0.5) * s); }
        else if constexpr (MODE == 1) { T s = 0; for (int i = 0; i < G::RE; ++i) { const T m = r[i].v + r[i].d[0]; s += m * m; } if (ok) acc += (double)(T(0.5) * s); }
        else {
            if (MODE == 3 && ok) { T s = 0; for (int i = 0; i < G::RE; ++i) s += r[i].d[0] * r[i].d[0]; acc += (double)s; }   // sum_u p_u (J^T J p)_u of this edge = |J p|^2 (o.t:2117-2122)
#pragma unroll
            for (int j = 0; j < G::V; ++j) {
#pragma unroll
                for (int k = 0; k < G::K; ++k) {
                    T gk = 0, dk = 0; bool any = false;
#pragma unroll
                    for (int i = 0; i < G::RE; ++i) {
                        if (!G::edgeDepends(i, j, k)) continue;
                        any = true;
                        const T d = r[i].d[(MODE == 3 ? 1 : 0) + j * G::K + k];
                        if (MODE == 2) { gk += d * r[i].v; dk += d * d; } else gk += d * r[i].d[0];
                    }
                    if (rec) {      // gather mode: record (slot j, hyperedge e), K (J^T J p) or 2 K (J^T F, then diag) scalars
                        if (ok) { constexpr int KK = MODE == 2 ? 2 * G::K : G::K; T* q = rec + ((long)j * nE + e) * KK; q[k] = gk; if (MODE == 2) q[G::K + k] = dk; }
                        continue;
                    }
                    if (!any) continue;
                    const long u = unknownIndex<T, G>(vo, X.vid[j], k);
                    if (j == 0) { segmentedAtomicAdd(out, u, MODE == 2 ? -gk : gk, ok); if (MODE == 2) segmentedAtomicAdd(diag, u, dk, ok); }
                    else if (ok) { plainAtomicAdd(out + u, MODE == 2 ? -gk : gk); if (MODE == 2) plainAtomicAdd(diag + u, dk); }
                }
            }
        }
    }
    if (MODE != 2) { const double t = blockReduceSum(acc, scratch); if (threadIdx.x == 0 && partials) partials[blockIdx.x] = t; }
}

// ---- two launches per PCG iteration (solver parameter amd_graph_fused = 1): [ge_flatStep: PCGStep2 + PCGStep3 of iteration k-1] + [ge_gather: PCGStep1 of iteration k] ----
// unknown k of vertex j of one hyperedge: component 0 = the solver vector, components 1..K = d/d(unknown k of ONE slot) -- where EdgeCtx seeds all V.
// J >= 0: that slot at compile time (derivative components no residual of the slot depends on fold away); J < 0: the member `slot` at run time (one body for every slot).
template <class T, class G, int J>
struct SlotCtx {
    typedef Dual<T, 1 + G::K> S;
    const G& g; long vid[G::V]; const T* vec; const GOff<G>& vo; int slot;
    __device__ __forceinline__ S operator()(int j, int k) const {
        S r(g.X[G::imgOf(k)][vid[j] * G::channels(G::imgOf(k)) + G::chOf(k)]);
        r.d[0] = vec[unknownIndex<T, G>(vo, vid[j], k)];
        if (j == (J >= 0 ? J : slot)) r.d[1 + k] = T(1);
        return r;
    }
};
// What ge_edges<T, G, 3> writes to the record of (slot, hyperedge e), computed instead of stored: forward-mode components do not interact, so the K derivative
// components seeded here carry the bits of components 1 + slot K .. of the edge pass.  jp2 (meaningful at slot 0): |J p|^2 of the hyperedge, its share of p . A p.
template <class T, class G, int J>
__device__ __forceinline__ void ge_slotRecord(const G& g, const GOff<G>& vo, const T* vec, long e, int slot, T (&q)[G::K], T& jp2) {
    typedef SlotCtx<T, G, J> Ctx;
    typedef typename Ctx::S S;
    const int js = J >= 0 ? J : slot;
    Ctx X{g, {}, vec, vo, js};
#pragma unroll
    for (int j = 0; j < G::V; ++j) X.vid[j] = g.vidx[j][e];
    S r[G::RE];
    g.template edgeResiduals<S>(X, e, r);
    if (J <= 0) { T s = 0; for (int i = 0; i < G::RE; ++i) s += r[i].d[0] * r[i].d[0]; jp2 = s; }
#pragma unroll
    for (int k = 0; k < G::K; ++k) {
        T gk = 0;
#pragma unroll
        for (int i = 0; i < G::RE; ++i) {
            if (!G::edgeDepends(i, js, k)) continue;
            gk += r[i].d[1 + k] * r[i].d[0];
        }
        q[k] = gk;
    }
}
// G::kSlotAtRunTime: the lanes of a wave walk entries of different slots, so V compile-time bodies run one after the other.  A functor whose hyperedge is expensive to
// evaluate (cotangent: four normalisations and two cotangents; robust: three sines and cosines) takes ONE body with the seeds chosen at run time instead; embedded, whose
// residuals are linear and whose slot-1 body folds to the three Offset components, keeps the V compile-time bodies.  The bits are the same either way.
template <class T, class G, int J = 0>
__device__ __forceinline__ void ge_slotDispatch(int j, const G& g, const GOff<G>& vo, const T* vec, long e, T (&q)[G::K], T& jp2) {
    if constexpr (G::kSlotAtRunTime) ge_slotRecord<T, G, -1>(g, vo, vec, e, j, q, jp2);
    else {
        if (j == J) ge_slotRecord<T, G, J>(g, vo, vec, e, J, q, jp2);
        else if constexpr (J + 1 < G::V) ge_slotDispatch<T, G, J + 1>(j, g, vo, vec, e, q, jp2);
    }
}
// out = J^T J vec (LM: + CtC vec) without records: ge_vertices<T, G, 3, GE_GATHER_LANES> with every record it would load evaluated in place -- the same lane split,
// the same ascending walk of the incidence list, the same shuffle fold, hence the same bits in `out`.  The edges' share of p . A p, |J p|^2 per hyperedge, is
// counted once: at the hyperedge's slot-0 entry.  S.r != nullptr: the launch is the Step1 half of a two-launch PCG iteration and adds the sums of graph_pcg.h IterSums,
// term by term, from the r and M = pre it is handed.
template <class T, class G, bool LM>
__global__ __launch_bounds__(kBlock) void ge_gather(G g, const T* __restrict__ vec, GOff<G> vo, T* __restrict__ out, const T* __restrict__ CtC, double* __restrict__ partials,
                                                     Incidence inc, IterSums<T> S) {
    constexpr int LANES = GE_GATHER_LANES;
    __shared__ double scratch[4 * (kBlock / kWave + 1)];
    double acc = 0, accNum = 0, acc2 = 0, acc3 = 0;
    const int sub = threadIdx.x % LANES;
    const int nE = g.nE;
    for (long v = (blockIdx.x * (long)blockDim.x + threadIdx.x) / LANES; v < g.N; v += (long)gridDim.x * blockDim.x / LANES) {
        typedef VertexCtx<T, G, true, true> Ctx;
        typedef typename Ctx::S SV;
        T gs[G::K];
        if (sub == 0) {
            SV r[G::RV > 0 ? G::RV : 1];
            g.template vertexResiduals<SV>(Ctx{g, v, vec, vo}, v, r);
#pragma unroll
            for (int k = 0; k < G::K; ++k) {
                T gk = 0;
#pragma unroll
                for (int i = 0; i < G::RV; ++i) gk += r[i].d[1 + k] * r[i].d[0];
                const long u = unknownIndex<T, G>(vo, v, k);
                if (LM) gk += CtC[u] * vec[u];
                acc += (double)(vec[u] * gk);
                gs[k] = gk;
            }
        } else {
#pragma unroll
            for (int k = 0; k < G::K; ++k) gs[k] = 0;
        }
        for (int t = inc.off[v] + sub, te = inc.off[v + 1]; t < te; t += LANES) {
            const int id = inc.idx[t], j = id / nE;
            T q[G::K], jp2 = 0;
            ge_slotDispatch<T, G>(j, g, vo, vec, (long)(id - j * nE), q, jp2);
            if (j == 0) acc += (double)jp2;
#pragma unroll
            for (int k = 0; k < G::K; ++k) gs[k] += q[k];
        }
#pragma unroll
        for (int off = LANES / 2; off > 0; off >>= 1)
#pragma unroll
            for (int k = 0; k < G::K; ++k) gs[k] += __shfl_down(gs[k], off, LANES);
        if (sub == 0) {
#pragma unroll
            for (int k = 0; k < G::K; ++k) {
                const long u = unknownIndex<T, G>(vo, v, k);
                out[u] = gs[k];
                if (S.r) { const double m = (double)S.M[u], rr = (double)S.r[u], a = (double)gs[k]; accNum += iterTerm(m, rr, rr); acc2 += iterTerm(m, rr, a); acc3 += iterTerm(m, a, a); }
            }
        }
    }
    if (S.r) { double vv[4] = {acc, accNum, acc2, acc3}; storeIterSums(vv, partials, S, scratch); return; }
    const double t = blockReduceSum(acc, scratch);
    if (threadIdx.x == 0 && partials) partials[blockIdx.x] = t;
}

// (PCGStep2 + PCGStep3 of the previous iteration in one flat pass: ge_flatStep, energy-independent, is graph_pcg.h's -- the stencil engine runs it too)

// ---- the whole linear solve in one workgroup (solver parameter amd_onchip = 6): the kernel and its variant list are graph_onchip.h, which the file that defines the
// functors includes behind this one ----
template <class T, class G>
struct GeOcArgs {
    G g; GOff<G> vo; long nScalars; Incidence inc; T* rec; int recInLds;      // rec: the plan's record buffer (K scalars per (slot, hyperedge) here); recInLds: the records live in LDS behind the vectors instead
    const T* r0; const T* p0; const T* M; T* delta;
    int L; double* trace;           // 4 doubles per iteration (alphaNum, alphaDen, s2, s3), or nullptr
    const T* CtC; T qTolerance; int resetPeriod; double* lmBreak;      // Levenberg-Marquardt
};
template <class T, class G> constexpr int geOcLdsVectors() { return G::kOnChipLdsVectors[sizeof(T) == 4 ? 0 : 1]; }      // solver vectors the kernel keeps in LDS: p, delta (2); r too (3); and A p (4)
struct GeOcVariant { int v; const void *gn, *lm; };      // V vertices per lane; nullptr: not offered
namespace { template <class T, class G> const std::vector<GeOcVariant>& geOcVariants(); }

// ---- the whole linear solve as one persistent launch of several workgroups (solver parameter amd_onchip = 7): the kernel is graph_onchip_grid.h ----
constexpr int kGeGridMaxG = 32;       // workgroup cap of the family
constexpr int kGeGridSumG = 64;       // ocGridSum's MAXG: it adds the workgroups' words a wave (64) at a time
constexpr int kGeGridRing = 4;        // halo scalars a lane collects per phase: a workgroup's halo is at most kGeGridRing * 512 scalars
struct GeGridPart {                   // one workgroup's part (graph_partition.h GraphPart), its lists as offsets into GeGridArgs::lists
    int nOwn, nHeld, nE, nRecv;       // owned / held vertices, hyperedges evaluated, halo scalars collected per phase
    int oHeld, oEdge, oSlot, oIncOff, oIncIdx, oWire;
    int oGidx;                        // [nHeld K]: the solver-vector index of every held scalar, bit 31 set on the halo
    int oRecv;                        // [nRecv][2]: {box index, held scalar} of every halo scalar
    long recBase;                     // the workgroup's slab of the record buffer, in records
};
template <class T, class G>
struct GeGridArgs {
    GeOcArgs<T, G> k;                 // what ge_onchipPcg is told, for the whole graph (inc unused; recInLds: every workgroup's records fit behind its vectors)
    int nG; const GeGridPart* parts; const int* lists;
    oc_u64 *slots, *box; long boxWords;      // [2][kGeGridSumG][2 NS] words of the sums, [2][boxWords] words of the wires
    unsigned tag0; int* bad; long long firstTicks, laterTicks; int failAt;
    int* hostErr;                     // LM: the pinned word a workgroup that gave up raises; Gauss-Newton: nullptr (ocApplyDelta tells the host)
};
struct GeGridKernels { const void *gn, *lm; };
namespace { template <class T, class G> GeGridKernels geGridKernels(); }

template <class T, class G>
struct GraphOps : EnergyOps<T> {
    G g{};
    GOff<G> vo{};
    int cus = 256;
    GraphOps(const unsigned* dims, bool usePre) {
        g.N = dims[0];
        this->usePreconditioner = usePre; this->usesGraph = true;
        for (int i = 0; i < G::NIMG; ++i) { vo.o[i] = this->nScalars; this->addUnknown(G::unknownParam(i), g.N, G::channels(i)); }
        int dev = 0; HIP_CHECK(hipGetDevice(&dev)); HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (const char* e = getenv("OPT_AMD_GRAPH_GATHER")) useGather = atoi(e) != 0;
        if (const char* e = getenv("OPT_AMD_ONCHIP_REC_LDS")) ocRecLds = atoi(e) != 0;
    }
    int vgrid(int lanes = 1) const { return (int)std::max<long>(1, std::min<long>((g.N * lanes + kBlock - 1) / kBlock, kMaxPartials / 2)); }
    // gather mode state: incidence lists (rebuilt when the graph arrays change: pointers, count or an order-independent checksum) and the record buffer
    bool useGather = true, gatherTooLarge = false;
    VertexLists inc; DevBuf<T> rec;      // rec: 2 K scalars per incidence (J^T F and diag; J^T J p uses K of them)
    Incidence incidence() const { return useGather ? Incidence{inc.off, inc.idx} : Incidence{nullptr, nullptr}; }
    void ensureLists(LaunchCtx& ctx) {
        SlotIdx<G::V> vi;
        for (int j = 0; j < G::V; ++j) vi.p[j] = g.vidx[j];
        if (!inc.ensure(vi, g.nE, g.N, cus, ctx, "buildIncidenceLists")) return;
        rec.reserve((size_t)std::max(1, g.nE) * G::V * 2 * G::K);
        ggBuiltG = 0;      // (the partition of amd_onchip = 7 follows the incidence lists)
    }
    void bind(void** p, LaunchCtx& ctx) override {
        g.bindParams(p);
        if (useGather && (long)g.nE * G::V > 0x7fffffffL) { useGather = false; gatherTooLarge = true; }      // incidence ids j * nE + e are 32-bit: beyond that, scatter
        if (useGather) ensureLists(ctx);
    }
    T* unknownPtr(int img) const override { return const_cast<T*>(g.X[img]); }
    void evalCost(Reduction& out, LaunchCtx& ctx) override {
        const int gv = vgrid(), ge = edgeGrid(g.nE, cus);
        { ScopedKernel k(ctx, "computeCost"); ge_vertices<T, G, 0><<<gv, kBlock, 0, ctx.stream>>>(g, nullptr, vo, nullptr, nullptr, nullptr, out.partials); }
        { ScopedKernel k(ctx, "computeCost_Graph"); ge_edges<T, G, 0><<<ge, kBlock, 0, ctx.stream>>>(g, nullptr, vo, nullptr, nullptr, out.partials + gv); }
        out.n = gv + ge;
    }
    void evalJTF(T* r, T* diag, LaunchCtx& ctx) override {
        if (useGather) {    // records first, then the vertex pass gathers them
            { ScopedKernel k(ctx, "PCGInit1_Graph"); ge_edges<T, G, 2><<<edgeGrid(g.nE, cus), kBlock, 0, ctx.stream>>>(g, nullptr, vo, r, diag, nullptr, rec); }
            { ScopedKernel k(ctx, "PCGInit1"); ge_vertices<T, G, 2, GE_GATHER_LANES><<<vgrid(GE_GATHER_LANES), kBlock, 0, ctx.stream>>>(g, nullptr, vo, r, diag, nullptr, nullptr, incidence(), rec); }
            return;
        }
        { ScopedKernel k(ctx, "PCGInit1"); ge_vertices<T, G, 2><<<vgrid(), kBlock, 0, ctx.stream>>>(g, nullptr, vo, r, diag, nullptr, nullptr); }
        { ScopedKernel k(ctx, "PCGInit1_Graph"); ge_edges<T, G, 2><<<edgeGrid(g.nE, cus), kBlock, 0, ctx.stream>>>(g, nullptr, vo, r, diag, nullptr); }
    }
    // ---- amd_graph_fused = 1 (EnergyOps::graphFused): J^T J p by ge_gather, the PCG iteration as ge_flatStep + ge_gather ----
    // THE predicate of the path: nullptr, or why the plan keeps the record kernels.  applyJTJ, pcgIteration and describe() all ask here.
    const char* fusedWhyNot() const {
        if (!useGather) return gatherTooLarge ? "more than 2^31 incidences (scatter mode)" : "scatter mode (OPT_AMD_GRAPH_GATHER=0)";
        return nullptr;
    }
    bool fusedOn() const { return this->graphFused && !fusedWhyNot(); }
    int launchGather(const T* v, T* out, const T* CtC, double* dotPartials, const IterSums<T>& S, LaunchCtx& ctx) {
        const int gv = vgrid(GE_GATHER_LANES);
        if (CtC) ge_gather<T, G, true><<<gv, kBlock, 0, ctx.stream>>>(g, v, vo, out, CtC, dotPartials, incidence(), S);
        else ge_gather<T, G, false><<<gv, kBlock, 0, ctx.stream>>>(g, v, vo, out, nullptr, dotPartials, incidence(), S);
        return gv;
    }
    bool pcgIteration(const PcgIterArgs<T>& a, LaunchCtx& ctx) override {
        if (!fusedOn() || !a.pre || this->slab.active || (a.CtC && !(a.b && a.q))) return false;
        const long nPad = (this->nScalars + 3) / 4 * 4;      // the solver's vectors (zero beyond nScalars)
        const int gf = flatGrid(nPad, cus, kMaxPartials / 2);
        pcgTwoLaunchIteration(a, nPad, ctx, [] {},
            [&](bool lm, const LmStep<T>& L) { return launchFlatStep<false>(a, nPad, gf, lm, L, nullptr, 0, ctx.stream); },
            [&](const IterSums<T>& S) { return launchGather(a.pNew, a.ApNew, a.CtC, a.aDen->partials, S, ctx); });
        return true;
    }
    // ---- the whole linear solve in ONE workgroup (graph_onchip.h; solver parameter amd_onchip = 6): gather mode, any vertex degree (the incidence lists are CSR), as many
    // vertices as a variant serves ----
    OnchipGuard ocGuard;      // the switches (OPT_AMD_ONCHIP = 0) and the failure word of the guarded update -- one ge_onchipPcg never sets (it has no wait that could time out) and ge_onchipPcgGrid does
    struct OcOffer { int v = 0; const void* fn = nullptr; };
    std::vector<OcOffer> ocOffers[2];      // [Gauss-Newton, Levenberg-Marquardt]: the variants this device can hold, smallest first
    bool ocReady = false;
    static constexpr size_t kOcLdsPerVertex = geOcLdsVectors<T, G>() * G::K * sizeof(T);      // p and delta (and r)
    static constexpr size_t kOcLdsBudget = 160 * 1024 - 512;      // dynamic LDS of a launch: the CU's 160 KB less the kernel's static staging of the sums (at most 448 bytes)
    bool ocRecLds = true;      // the records of an iteration live in LDS where they fit beside the vectors (OPT_AMD_ONCHIP_REC_LDS=0, read per plan: always the plan's buffer; the A/B switch of profiles/onchip_graph.md)
    // dynamic LDS of a launch on the graph as bound: the vectors, then the records if there is room
    size_t ocLdsBytes(bool* recInLds) const {
        const size_t vec = (size_t)g.N * kOcLdsPerVertex, recBytes = (size_t)std::max(1, g.nE) * G::V * G::K * sizeof(T);
        const bool in = ocRecLds && vec + recBytes <= kOcLdsBudget;
        if (recInLds) *recInLds = in;
        return (vec + (in ? recBytes : 0) + 15) / 16 * 16;
    }
    void ocInit() {
        if (ocReady) return;
        ocReady = true;
        for (const GeOcVariant& v : geOcVariants<T, G>())
            for (int m = 0; m < 2; ++m) {
                const void* fn = m ? v.lm : v.gn;
                if ((size_t)v.v * kOcWgMaxBlock * kOcLdsPerVertex > kOcLdsBudget) continue;      // (a variant whose largest mesh the CU cannot hold is not offered)
                if (ocOfferable(fn, kOcLdsBudget)) ocOffers[m].push_back({v.v, fn});
            }
    }
    long ocMaxVertices(bool lmv) { ocInit(); return ocOffers[lmv].empty() ? 0 : (long)ocOffers[lmv].back().v * kOcWgMaxBlock; }
    // THE predicate of the path: nullptr (on chip, *pick = the variant) or why the plan keeps its launch-per-iteration loop.  pcgSolveOnChip and describe() both ask here.
    // (what any on-chip solve of the family needs, one workgroup or several)
    const char* ocCommonWhyNot(int L, bool lmv, const OnChipLm<T>* lm) const {
        if (this->onChipLevel < 6) return "amd_onchip=6 was not set";
        if (ocGuard.whyOff()) return ocGuard.whyOff();
        if (fusedWhyNot()) return fusedWhyNot();      // scatter mode: no incidence lists, no records
        if (!this->usePreconditioner || !this->onChipPre) return "no preconditioner vector";
        if (this->slab.active) return "row slabs";
        if (L <= 0) return "no PCG iterations";
        if (lmv && lm && !lm->CtC) return "no LM diagonal";
        if (g.N < 1) return "no vertices";
        return nullptr;
    }
    const char* ocWhyNot(int L, bool lmv, const OnChipLm<T>* lm, const OcOffer** pick = nullptr) {
        if (const char* why = ocCommonWhyNot(L, lmv, lm)) return why;
        ocInit();
        for (const OcOffer& o : ocOffers[lmv])
            if (g.N <= (long)o.v * kOcWgMaxBlock) { if (pick) *pick = &o; return nullptr; }
        return "too many vertices";
    }
    // ---- ... or as ONE persistent launch of several workgroups (graph_onchip_grid.h; solver parameter amd_onchip = 7, amd_onchip_workgroups) ----
    GraphPartition ggPart;            // the partition in force (host copy: describe() reports from it)
    int ggBuiltG = 0;                 // its workgroup count; 0: none (the graph has changed: ensureLists)
    DevBuf<GeGridPart> ggParts; DevBuf<int> ggLists;
    DevBuf<T> ggRec;      // the workgroups' record slabs (K scalars per evaluated (hyperedge, slot)), used where the records do not fit LDS
    oc_u64 *ggSlots = nullptr, *ggBox = nullptr; long ggBoxWords = 0, ggBoxCap = 0;
    const void* ggFn[2] = {nullptr, nullptr}; bool ggReady = false;
    static constexpr size_t kGgLdsPerVertex = 4 * G::K * sizeof(T);      // p, delta, r, A p
    static constexpr size_t kGgLdsBudget = 160 * 1024 - 4096;            // dynamic LDS of a launch: the CU's 160 KB less the kernel's static staging of the sums (OcSumLds for 64 workgroups: at most 2928 bytes)
    // Automatic workgroup count (amd_onchip_workgroups = 0): the rule of profiles/onchip_graph_grid.md, which names a workload only where the several-workgroup launch
    // was MEASURED faster than every other setting (median below the minimum of the best of them).  Measured there: 130 .. 2000 vertices, 768 .. 12108 hyperedges, and at
    // every size the full 32 workgroups were the fastest count.  So: 32 workgroups from kGgAutoMinVertices up to the functor's G::kOnChipGridAutoMaxVertices[precision]
    // (2000, the largest mesh measured; cotangent in double: 689 -- it lost on the raptor), one workgroup (level 6's behaviour) elsewhere.  A plan the several-workgroup
    // predicate refuses under the automatic choice (LDS, ring, entanglement) does what level 6 does as well.
    static constexpr long kGgAutoMinVertices = 130;
    int ggAutoWorkgroups() const { return g.N >= kGgAutoMinVertices && g.N <= G::kOnChipGridAutoMaxVertices[sizeof(T) == 4 ? 0 : 1] ? kGeGridMaxG : 1; }
    bool ggForced() const { return this->onChipWorkgroups > 0; }
    // the workgroup count level 7 asks for on the graph as bound (1: the one-workgroup path)
    int ggWanted() const {
        if (this->onChipLevel < 7 || g.N < 1) return 1;
        return graphPartitionClamp(g.N, this->onChipWorkgroups > 0 ? this->onChipWorkgroups : ggAutoWorkgroups(), kGeGridMaxG);
    }
    void ggInit() {
        if (ggReady) return;
        ggReady = true;
        const GeGridKernels ks = geGridKernels<T, G>();
        for (int m = 0; m < 2; ++m)
            if (const void* fn = m ? ks.lm : ks.gn; ocOfferable(fn, kGgLdsBudget)) ggFn[m] = fn;
    }
    // the partition for G workgroups on the graph as bound, on the device (blocking copies: once per graph and workgroup count)
    void ggEnsure(int G_) {
        if (ggBuiltG == G_) return;
        std::vector<int> h[G::V]; const int* hp[G::V];
        for (int j = 0; j < G::V; ++j) {
            h[j].resize((size_t)std::max(1, g.nE));
            if (g.nE > 0) HIP_CHECK(hipMemcpy(h[j].data(), g.vidx[j], (size_t)g.nE * sizeof(int), hipMemcpyDeviceToHost));
            hp[j] = h[j].data();
        }
        ggPart = buildGraphPartition(g.N, g.nE, G::V, hp, G_);
        std::vector<int> lists; std::vector<GeGridPart> parts((size_t)G_);
        auto put = [&](const std::vector<int>& v) { const int o = (int)lists.size(); lists.insert(lists.end(), v.begin(), v.end()); return o; };
        long recBase = 0;
        for (int w = 0; w < G_; ++w) {
            const GraphPart& Q = ggPart.parts[(size_t)w]; GeGridPart& D = parts[(size_t)w];
            const int nHeld = (int)Q.held.size(), nHalo = nHeld - Q.nOwn;
            D.nOwn = Q.nOwn; D.nHeld = nHeld; D.nE = (int)Q.edge.size(); D.nRecv = nHalo * G::K; D.recBase = recBase;
            recBase += (long)D.nE * G::V;
            D.oHeld = put(Q.held); D.oEdge = put(Q.edge); D.oSlot = put(Q.slot); D.oIncOff = put(Q.incOff); D.oIncIdx = put(Q.incIdx); D.oWire = put(Q.wire);
            GOff<G> lo; { long o = 0; for (int i = 0; i < G::NIMG; ++i) { lo.o[i] = o; o += (long)nHeld * G::channels(i); } }
            std::vector<int> gidx((size_t)nHeld * G::K), recv((size_t)nHalo * G::K * 2);
            for (int l = 0; l < nHeld; ++l)
                for (int k = 0; k < G::K; ++k) {
                    const long ul = lo.o[G::imgOf(k)] + (long)l * G::channels(G::imgOf(k)) + G::chOf(k), ug = vo.o[G::imgOf(k)] + (long)Q.held[(size_t)l] * G::channels(G::imgOf(k)) + G::chOf(k);
                    gidx[(size_t)ul] = (int)ug | (l < Q.nOwn ? 0 : (int)0x80000000);
                    if (l >= Q.nOwn) { const size_t hh = (size_t)(l - Q.nOwn) * G::K + k; recv[2 * hh] = Q.haloWire[(size_t)(l - Q.nOwn)] * G::K + k; recv[2 * hh + 1] = (int)ul; }
                }
            D.oGidx = put(gidx); D.oRecv = put(recv);
        }
        lists.push_back(0);      // (never empty)
        HIP_CHECK(hipDeviceSynchronize());      // (no launch still reads the lists about to be replaced)
        ggLists.reserve(lists.size()); ggParts.reserve(kGeGridMaxG); ggRec.reserve((size_t)recBase * G::K);
        HIP_CHECK(hipMemcpy(ggLists, lists.data(), lists.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ggParts, parts.data(), parts.size() * sizeof(GeGridPart), hipMemcpyHostToDevice));
        // the tagged words, allocated once per plan: the sums' slots, and the wires' box at its worst case -- every unknown on a wire (a fresh buffer starts cleared: zero is no tag)
        if (!ggSlots) { const size_t b = sizeof(oc_u64) * 2 * kGeGridSumG * 2 * 5; ggSlots = ocGuard.template allocTagged<oc_u64>(b); HIP_CHECK(hipMemset(ggSlots, 0, b)); }
        ggBoxWords = std::max<long>(1, (long)ggPart.nWires * G::K * (long)(sizeof(T) / 4));
        if (!ggBox) { ggBoxCap = std::max<long>(1, this->nScalars * (long)(sizeof(T) / 4)); const size_t b = sizeof(oc_u64) * 2 * (size_t)ggBoxCap; ggBox = ocGuard.template allocTagged<oc_u64>(b); HIP_CHECK(hipMemset(ggBox, 0, b)); }
        ggBuiltG = G_;
    }
    // dynamic LDS of a launch on the partition in force: the vectors of the largest part, then the records of the largest part if there is room
    size_t ggLdsBytes(bool* recInLds) const {
        const size_t vec = (size_t)ggPart.heldMax * kGgLdsPerVertex, recBytes = (size_t)std::max(1, ggPart.edgesMax) * G::V * G::K * sizeof(T);
        const bool in = ocRecLds && vec + recBytes <= kGgLdsBudget;
        if (recInLds) *recInLds = in;
        return (vec + (in ? recBytes : 0) + 15) / 16 * 16;
    }
    // Redundant evaluation the AUTOMATIC choice allows, as evaluated / total hyperedges: 11 / 4.  The largest ratio measured is 2.68 (cotangent, 130 vertices on 32
    // workgroups: still faster than every other setting, profiles/onchip_graph_grid.md); beyond what was measured the automatic choice does not go.  A caller who
    // forces a workgroup count is not held to it.
    static constexpr long kGgEntangledNum = 11, kGgEntangledDen = 4;
    // THE predicate of the several-workgroup path: nullptr (on chip with G_ workgroups, the partition built) or why not.  pcgSolveOnChip and describe() both ask here.
    const char* ggWhyNot(int L, bool lmv, const OnChipLm<T>* lm, int G_) {
        if (const char* why = ocCommonWhyNot(L, lmv, lm)) return why;
        if (!inc.valid) return "no graph bound yet";
        if (this->nScalars > 0x7fffffffL / 2) return "too many unknowns";
        ggInit();
        if (!ggFn[lmv]) return "the kernel is not offered on this device (scratch)";
        ggEnsure(G_);
        if ((size_t)ggPart.heldMax * kGgLdsPerVertex > kGgLdsBudget) return "held vertices do not fit LDS";
        if ((long)ggPart.haloMax * G::K > (long)kGeGridRing * kOcWgMaxBlock) return "a part's halo does not fit the ring";
        if (!ggForced() && kGgEntangledDen * ggPart.evaluated > kGgEntangledNum * (long)std::max(1, g.nE)) return "partition too entangled";
        return nullptr;
    }
    bool ggSolve(const T* r0, const T* p0, T* delta, int L, double* traceDev, const OnChipLm<T>* lm, int G_, LaunchCtx& ctx) {
        if (ggWhyNot(L, lm != nullptr, lm, G_) || (lm && !lm->CtC)) return false;
        bool recInLds = false;
        const size_t lds = ggLdsBytes(&recInLds);
        ocGuard.allocWords(ctx.stream);
        const int period = lm ? lm->resetPeriod : 0, phases = L + (period > 0 ? (L - 1) / period : 0);
        const OcTimeouts tmo = ocGuard.timeouts(phases, false);
        GeGridArgs<T, G> A{};
        A.k = GeOcArgs<T, G>{g, vo, this->nScalars, incidence(), ggRec, recInLds ? 1 : 0, r0, p0, this->onChipPre, delta, L, traceDev, lm ? lm->CtC : nullptr, lm ? lm->qTolerance : T(0), period,
                             lm ? lm->breakInfo : nullptr};
        A.nG = G_; A.parts = ggParts; A.lists = ggLists; A.slots = ggSlots; A.box = ggBox; A.boxWords = ggBoxWords;
        A.tag0 = ocGuard.tags((unsigned)phases, ctx.stream); A.bad = ocGuard.bad; A.firstTicks = tmo.first; A.laterTicks = tmo.later; A.failAt = ocGuard.failAtThisLaunch();
        A.hostErr = lm ? ocGuard.hostErr : nullptr;
        void* kargs[] = {(void*)&A};
        return ocLaunchSolve(ggFn[lm ? 1 : 0], dim3(G_), dim3(kOcWgMaxBlock), kargs, lds, ocGuard, *this, delta, lm != nullptr, ctx);
    }
    bool pcgSolveOnChip(const T* r0, const T* p0, T* delta, int L, double* traceDev, const OnChipLm<T>* lm, LaunchCtx& ctx) override {
        if (const int G_ = ggWanted(); G_ > 1) {
            if (ggForced() || !ggWhyNot(L, lm != nullptr, lm, G_)) return ggSolve(r0, p0, delta, L, traceDev, lm, G_, ctx);
        }      // (the automatic choice refused: what level 6 does)
        const OcOffer* o = nullptr;
        if (ocWhyNot(L, lm != nullptr, lm, &o) || (lm && !lm->CtC)) return false;
        // only the waves the mesh needs: those its vertices fill at V per lane, and as many more (up to 8) as its hyperedges fill in the edge phase
        const int threads = std::max(1, std::max(divUp(divUp(g.N, o->v), kWave), std::min(kOcWgMaxWaves, divUp(g.nE, kWave)))) * kWave;
        bool recInLds = false;
        const size_t lds = ocLdsBytes(&recInLds);
        GeOcArgs<T, G> K{g, vo, this->nScalars, incidence(), rec, recInLds ? 1 : 0, r0, p0, this->onChipPre, delta, L, traceDev, lm ? lm->CtC : nullptr, lm ? lm->qTolerance : T(0), lm ? lm->resetPeriod : 0,
                         lm ? lm->breakInfo : nullptr};
        void* kargs[] = {(void*)&K};
        return ocLaunchSolve(o->fn, dim3(1), dim3(threads), kargs, lds, ocGuard, *this, delta, lm != nullptr, ctx);
    }
    OnchipGuard* onChipGuard() override { return &ocGuard; }
    // ("key=value; ..." -- no ';' inside a value.)  At level 7 with more than one workgroup asked for, the answer needs the partition: the first call for a graph and
    // workgroup count builds it here (ggEnsure: a device synchronisation and blocking copies of the index arrays), exactly as the first solve would.
    std::string describe(int L, bool lmv, const OnChipLm<T>* lm) override {
        const char* prec = sizeof(T) == 4 ? "float" : "double";
        char buf[500];
        std::string ocWhy;      // amd_onchip >= 6 and the plan is refused: why
        const int G_ = ggWanted();
        const char* ggWhy = G_ > 1 ? ggWhyNot(L, lmv, lm, G_) : nullptr;
        if (G_ > 1 && (ggForced() || !ggWhy)) {      // amd_onchip = 7 and more than one workgroup: forced, or chosen and taken (a refused automatic choice does what level 6 does)
            const char* why = ggWhy;
            if (!why) {
                bool recInLds = false;
                (void)ggLdsBytes(&recInLds);
                snprintf(buf, sizeof buf, "path=on-chip; workgroups=%d; vertices=%ld; hyperedges=%d; evaluated_hyperedges=%ld; held_vertices_max=%d; variant=ge_onchipPcgGrid<%s, %s, %s>; records=%s", G_, g.N,
                         g.nE, ggPart.evaluated, ggPart.heldMax, prec, G::kName, lmv ? "LM" : "GN", recInLds ? "LDS" : "memory");
                return buf;
            }
            ocWhy = std::string("; why_not_on_chip=") + why + " (workgroups=" + std::to_string(G_) + ")";
        } else if (this->onChipLevel >= 6) {
            const OcOffer* o = nullptr;
            const char* why = ocWhyNot(L, lmv, lm, &o);
            if (!why) {
                bool recInLds = false;
                (void)ocLdsBytes(&recInLds);
                snprintf(buf, sizeof buf, "path=on-chip; workgroups=1; vertices=%ld; hyperedges=%d; variant=ge_onchipPcg<%s, %s, %d, %s>; records=%s", g.N, g.nE, prec, G::kName, o->v, lmv ? "LM" : "GN",
                         recInLds ? "LDS" : "memory");
                return buf;
            }
            ocWhy = std::string("; why_not_on_chip=") + why;
            if (!strcmp(why, "too many vertices")) ocWhy += " (the variants serve up to " + std::to_string(ocMaxVertices(lmv)) + ")";
        }
        if (!this->graphFused) return "path=launch-per-iteration" + ocWhy;
        const char* why = fusedWhyNot();
        if (!why && !this->usePreconditioner) why = "no preconditioner";
        if (why) snprintf(buf, sizeof buf, "path=launch-per-iteration; why_not_fused=%s", why);
        else snprintf(buf, sizeof buf, "path=launch-per-iteration; launches_per_iteration=2; kernels=ge_flatStep+ge_gather<%s, %s, %s>", prec, G::kName, lmv ? "LM" : "GN");
        return buf + ocWhy;
    }
    void applyJTJ(const T* v, T* out, const T* CtC, Reduction* dot, LaunchCtx& ctx) override {
        if (fusedOn()) {      // one launch instead of two, the same bits in `out`
            ScopedKernel k(ctx, "PCGStep1");
            const int gv = launchGather(v, out, CtC, dot ? dot->partials : nullptr, IterSums<T>{nullptr, nullptr, nullptr, nullptr, nullptr}, ctx);
            if (dot) dot->n = gv;
            return;
        }
        const int gv = vgrid(useGather ? GE_GATHER_LANES : 1), ge = edgeGrid(g.nE, cus);
        if (useGather) {
            { ScopedKernel k(ctx, "PCGStep1_Graph"); ge_edges<T, G, 3><<<ge, kBlock, 0, ctx.stream>>>(g, v, vo, out, nullptr, dot ? dot->partials + gv : nullptr, rec); }
            { ScopedKernel k(ctx, "PCGStep1"); ge_vertices<T, G, 3, GE_GATHER_LANES><<<gv, kBlock, 0, ctx.stream>>>(g, v, vo, out, nullptr, CtC, dot ? dot->partials : nullptr, incidence(), rec); }
            if (dot) dot->n = gv + ge;
            return;
        }
        { ScopedKernel k(ctx, "PCGStep1"); ge_vertices<T, G, 3><<<gv, kBlock, 0, ctx.stream>>>(g, v, vo, out, nullptr, CtC, dot ? dot->partials : nullptr); }
        { ScopedKernel k(ctx, "PCGStep1_Graph"); ge_edges<T, G, 3><<<ge, kBlock, 0, ctx.stream>>>(g, v, vo, out, nullptr, dot ? dot->partials + gv : nullptr); }
        if (dot) dot->n = gv + ge;
    }
    void evalModelCost(const T* delta, Reduction& out, LaunchCtx& ctx) override {
        const int gv = vgrid(), ge = edgeGrid(g.nE, cus);
        { ScopedKernel k(ctx, "computeModelCost"); ge_vertices<T, G, 1><<<gv, kBlock, 0, ctx.stream>>>(g, delta, vo, nullptr, nullptr, nullptr, out.partials); }
        { ScopedKernel k(ctx, "computeModelCost_Graph"); ge_edges<T, G, 1><<<ge, kBlock, 0, ctx.stream>>>(g, delta, vo, nullptr, nullptr, out.partials + gv); }
        out.n = gv + ge;
    }
};

}  // namespace optamd
