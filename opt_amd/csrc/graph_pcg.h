// What the PCG kernels of the graph kernel sets share, each piece written once: the value types and derivative columns of ARAP's gather (arap_applyEll, arap_onchipPcg;
// the body of the walk is arap_half_edge_pair.inc), the argument structs, the term and the store of the sums of a two-launch iteration (arap_applyEll, ge_gather,
// arap_onchipPcg), LM's extras of the flat PCGStep2 + PCGStep3 pass (arap_flatStepPlanes, ge_flatStep; its scalars are graph_flat_scalars.inc) and the host side of
// such an iteration (ArapOps::pcgIteration, GraphOps::pcgIteration, StencilOps::pcgIteration) -- and, at the end of the file, the two energy-independent kernels of
// that pass themselves, ge_flatStep and ge_flatStepNoPre, which both functor engines launch (graph_engine.h, stencil_engine.h) through launchFlatStep.  Every device piece is a force-inlined
// function on plain values; a kernel keeps its own loop, layout,
// grid and walk order, and the order in which it adds the terms it gets from here.  No pragma in this file: it is compiled with the contraction setting of the file
// that includes it (energy_graph_functors.hip and plug-in sources: off; energy_functors.hip: the compiler's default).  The kernels take LmStep, a type of this file's
// unnamed namespace, so every translation unit launches its own copy.  Every kernel but arap_applyFused, which lost dead code, compiles to the instructions it had before these pieces
// were shared; what else was tried as a function, and what the compiler made of it: profiles/graph_shared_text.md.
#pragma once
#include "graph_common.h"

namespace optamd {
namespace {

template <class T> struct V3 { T x, y, z; };
template <class T> __device__ __forceinline__ T dot3(const V3<T>& a, const V3<T>& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <class T> __device__ __forceinline__ V3<T> ldv3(const T* p, long i) { return reinterpret_cast<const V3<T>*>(p)[i]; }      // one 12 / 24-byte load
template <class T> __device__ __forceinline__ void stv3(T* p, long i, const V3<T>& v) { reinterpret_cast<V3<T>*>(p)[i] = v; }
template <class T> struct alignas(16) Q4 { T a, b, c, d; };      // an entry of a 16-byte (double: 32-byte) SoA plane

// ---- ARAP: J^T J p at a vertex -------------------------------------------------------------------------------------------------------------------------------
template <class T> struct ArapCoef { T a0, a1, a2, a3, a4, a5, b0, b1, b2, b3, b4, b5, b6, b7, b8, c0, c1, c2, c3, c4, c5; };
// the non-zero entries of dR3/d alpha, d beta, d gamma (arap_rot's coefficients, same products)
template <class T>
__device__ __forceinline__ ArapCoef<T> arap_coef(T sa, T ca, T sb, T cb, T sg, T cg) {
    ArapCoef<T> c;
    c.a0 = sg * sa + cg * sb * ca;  c.a1 = sg * ca - cg * sb * sa;
    c.a2 = -cg * sa + sg * sb * ca; c.a3 = -cg * ca - sg * sb * sa;
    c.a4 = cb * ca;                 c.a5 = -cb * sa;
    c.b0 = -cg * sb; c.b1 = cg * cb * sa; c.b2 = cg * cb * ca;
    c.b3 = -sg * sb; c.b4 = sg * cb * sa; c.b5 = sg * cb * ca;
    c.b6 = -cb;      c.b7 = -sb * sa;     c.b8 = -sb * ca;
    c.c0 = -sg * cb; c.c1 = -cg * ca - sg * sb * sa; c.c2 = cg * sa - sg * sb * ca;
    c.c3 = cg * cb;  c.c4 = -sg * ca + cg * sb * sa; c.c5 = sg * sa + cg * sb * ca;
    return c;
}
template <class T>
__device__ __forceinline__ void arap_cols(const ArapCoef<T>& c, const V3<T>& u, V3<T>& D0, V3<T>& D1, V3<T>& D2) {
    D0.x = c.a0 * u.y + c.a1 * u.z; D0.y = c.a2 * u.y + c.a3 * u.z; D0.z = c.a4 * u.y + c.a5 * u.z;
    D1.x = c.b0 * u.x + c.b1 * u.y + c.b2 * u.z; D1.y = c.b3 * u.x + c.b4 * u.y + c.b5 * u.z; D1.z = c.b6 * u.x + c.b7 * u.y + c.b8 * u.z;
    D2.x = c.c0 * u.x + c.c1 * u.y + c.c2 * u.z; D2.y = c.c3 * u.x + c.c4 * u.y + c.c5 * u.z; D2.z = 0;
}
// ---- the sums of a two-launch PCG iteration ----------------------------------------------------------------------------------------------------------------------
// S.r != nullptr: the gather is the Step1 half of a two-launch iteration ([flat PCGStep2 + PCGStep3 pass] + [gather]; EnergyOps::pcgIteration).  Besides p . A p it then
// sums, at the lane that owns the vertex, what the next flat pass needs -- alphaNumerator = sum M r^2 and the two sums of the expanded beta numerator, s2 = sum M r . A p and
// s3 = sum M (A p)^2 (energy.h PcgIterArgs), every term from M, r, A p themselves in double (exact products of floats; see energy_image_warping.hip dprod3) -- so that
// PCGStep2 and PCGStep3 become one flat pass without a reduction between them.
template <class T> struct IterSums { const T* r; const T* M; double *aNum, *s2, *s3; };
template <class T> __device__ __forceinline__ double iterTerm(T m, T a, T b) { return ((double)m * (double)a) * (double)b; }
// the end of such a gather: vv = {p . A p, aNum, s2, s3} over the workgroup, one partial each.  scratch: 4 * blockDim / 64 doubles.  (vv is the caller's: with the array
// inside this function the partial-sum loop of ge_gather came out with its branch turned round)
template <class T>
__device__ __forceinline__ void storeIterSums(double (&vv)[4], double* partials, const IterSums<T>& S, double* scratch) {
    blockReduceSumN<4>(vv, scratch);
    if (threadIdx.x == 0) { if (partials) partials[blockIdx.x] = vv[0]; S.aNum[blockIdx.x] = vv[1]; S.s2[blockIdx.x] = vv[2]; S.s3[blockIdx.x] = vv[3]; }
}

// ---- the flat pass: PCGStep2 + PCGStep3 of the previous iteration (solver.t:446-489, 537-550) ---------------------------------------------------------------------------
// LM (Levenberg-Marquardt): delta goes to deltaOut (the solver enqueues the next launch before it has read Q: an early-out must still find the old delta),
// Q_{k-1} = 1/2 sum delta . (r + b) (solver.t:483-485) leaves as per-workgroup partials (tagged words if qTag != 0), and after a split residual reset (afterReset: delta
// and r are already the new ones, solver.t:1077-1083) the pass only forms p = M r + beta p with beta = sum bNum / sum bDen.
template <class T> struct LmStep { const T* b; T* deltaOut; double* q; unsigned qTag; int afterReset; const double* bNumP; int nbNum; const double* bDenP; int nbDen; };
// The scalars of the pass -- alpha, beta, restart -- are graph_flat_scalars.inc: text both kernels include, not a function (see there).

// ---- host side of a two-launch iteration -------------------------------------------------------------------------------------------------------------------------------
// first(): what the first launch of a solve needs besides the start state; flat(lm, L): launches the flat pass and returns its grid; gather(S): launches the gather and
// returns its grid.  nPad: the scalars of the solver's vectors.
template <class T, class First, class Flat, class Gather>
void pcgTwoLaunchIteration(const PcgIterArgs<T>& a, long nPad, LaunchCtx& ctx, First&& first, Flat&& flat, Gather&& gather) {
    const bool lmv = a.CtC != nullptr;
    if (a.first) {      // the solver adopts rNew / pNew after every launch: the start state moves there unchanged
        HIP_CHECK(hipMemcpyAsync(a.rNew, a.rOld, nPad * sizeof(T), hipMemcpyDeviceToDevice, ctx.stream));
        HIP_CHECK(hipMemcpyAsync(a.pNew, a.pOld, nPad * sizeof(T), hipMemcpyDeviceToDevice, ctx.stream));
        first();
    } else {
        ScopedKernel k(ctx, "PCGStep2+PCGStep3");
        const LmStep<T> L = lmv ? LmStep<T>{a.b, a.deltaOut ? a.deltaOut : a.delta, a.q->partials, a.qTag, a.afterReset, a.betaNum.partials, a.betaNum.n, a.betaDen.partials, a.betaDen.n} : LmStep<T>{};
        const int g = flat(lmv, L);
        if (lmv && !a.afterReset) a.q->n = g;
    }
    ScopedKernel k(ctx, "PCGStep1");
    const int g = gather(IterSums<T>{a.rNew, a.pre, a.aNum->partials, a.s2->partials, a.s3->partials});
    a.aNum->n = a.aDen->n = a.s2->n = a.s3->n = g;
}

}  // namespace

// PCGStep2 + PCGStep3 of the previous iteration in one flat pass over the padded scalars: the scalars of graph_flat_scalars.inc, LM's extras (LmStep), the
// update in a grid-stride loop.  Energy-independent: arap_flatStepPlanes without the planes.  Launched by both functor engines (graph_engine.h GraphOps::pcgIteration,
// stencil_engine.h StencilOps::pcgIteration).
template <class T, bool LM>
__global__ __launch_bounds__(kBlock) void ge_flatStep(long n, T* __restrict__ delta, const T* __restrict__ pOld, const T* __restrict__ rOld, const T* __restrict__ Ap, const T* __restrict__ M,
                                                       T* __restrict__ rNew, T* __restrict__ pNew, const double* aNumP, int nNum, const double* aDenP, int nDen,
                                                       const double* s2P, int n2, const double* s3P, int n3, LmStep<T> L) {
    __shared__ double scratch[4 * (kBlock / kWave + 1)];
#include "graph_flat_scalars.inc"      // alpha, beta, restart
    T* const dOut = LM ? L.deltaOut : delta;
    double accQ = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const T p = pOld[i], r = rOld[i], m = M[i];
        T rn, pn;
        if (restart) { rn = r; pn = m * r + beta * p; }
        else {
            const T d = delta[i] + alpha * p;
            rn = r - alpha * Ap[i];
            const T z = m * rn;
            pn = z + beta * p;
            if (LM) accQ += (double)(T(0.5) * (d * (rn + L.b[i])));
            dOut[i] = d;
        }
        rNew[i] = rn; pNew[i] = pn;
    }
    if (LM && L.q && !restart) {
        const double tq = blockReduceSum(accQ, scratch);
        if (threadIdx.x == 0) { if (L.qTag) storeTaggedPartial(L.q, blockIdx.x, tq, L.qTag); else L.q[blockIdx.x] = tq; }
    }
}

// The same pass for an energy that does not precondition (UsePreconditioner(false): the solver hands pcgIteration no M): M == 1 at compile time, no load of it.
// The first pass of a linear solve differs from the later ones in one scalar.  The reference starts such a solve from p_0 = M_0 r_0 with a vector M_0 that is not 1
// (PCGInit1: guardedInvert(1) = 1/4; Levenberg-Marquardt: PCGFinalizeDiagonal's preconditioner) and alphaNumerator_0 = r_0 . p_0, and continues with z = r.  The
// gather of the first launch therefore leaves r_0 . p_0 as its alphaNumerator -- what alpha_0 = aNum / aDen and beta_0's denominator are -- and sum r_0^2, which the
// expansion of beta_0's numerator sum (r_0 - alpha A p_0)^2 = sum r_0^2 - 2 alpha s2 + alpha^2 s3 starts from, apart in rr0P (nullptr on every later pass, where
// the two are the same sum).  The arithmetic is graph_flat_scalars.inc's with that one term exchanged; the restart after a split residual reset is unchanged.
template <class T, bool LM>
__global__ __launch_bounds__(kBlock) void ge_flatStepNoPre(long n, T* __restrict__ delta, const T* __restrict__ pOld, const T* __restrict__ rOld, const T* __restrict__ Ap,
                                                            T* __restrict__ rNew, T* __restrict__ pNew, const double* aNumP, int nNum, const double* aDenP, int nDen,
                                                            const double* s2P, int n2, const double* s3P, int n3, const double* rr0P, int nrr0, LmStep<T> L) {
    __shared__ double scratch[4 * (kBlock / kWave + 1)];
    T alpha, beta;
    const bool restart = LM && L.afterReset;
    if (restart) {
        const double* const ps[2] = {L.bNumP, L.bDenP}; const int ns[2] = {L.nbNum, L.nbDen}; double o2[2];
        sumPartialsN<2>(ps, ns, scratch, o2);
        const T bNum = (T)o2[0], bDen = (T)o2[1];
        alpha = T(0); beta = (bDen > T(0)) ? bNum / bDen : T(0);                            // PCGStep3's guard (solver.t:544-547)
    } else {
        const double* const ps[4] = {aNumP, aDenP, s2P, s3P}; const int ns[4] = {nNum, nDen, n2, n3}; double o4[4];
        sumPartialsN<4>(ps, ns, scratch, o4);
        const double rr = rr0P ? sumPartials(rr0P, nrr0, scratch) : o4[0];                   // (a kernel argument: uniform)
        const T aNum = (T)o4[0], aDen = (T)o4[1];
        alpha = (aDen > T(0)) ? aNum / aDen : T(0);                                          // solver.t:456-459
        const double bNumD = fmax(rr - 2.0 * (double)alpha * o4[2] + (double)alpha * (double)alpha * o4[3], 0.0);
        beta = (aNum > T(0)) ? (T)bNumD / aNum : T(0);                                       // solver.t:544-547
    }
    T* const dOut = LM ? L.deltaOut : delta;
    double accQ = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const T p = pOld[i], r = rOld[i];
        T rn, pn;
        if (restart) { rn = r; pn = r + beta * p; }
        else {
            const T d = delta[i] + alpha * p;
            rn = r - alpha * Ap[i];
            pn = rn + beta * p;
            if (LM) accQ += (double)(T(0.5) * (d * (rn + L.b[i])));
            dOut[i] = d;
        }
        rNew[i] = rn; pNew[i] = pn;
    }
    if (LM && L.q && !restart) {
        const double tq = blockReduceSum(accQ, scratch);
        if (threadIdx.x == 0) { if (L.qTag) storeTaggedPartial(L.q, blockIdx.x, tq, L.qTag); else L.q[blockIdx.x] = tq; }
    }
}

namespace {
// The launch of the flat pass from the arguments of an iteration (the flat(lm, L) of pcgTwoLaunchIteration): ge_flatStep, or for an energy that does not
// precondition (a.pre == nullptr) ge_flatStepNoPre with the first launch's sum r_0^2 (rr0, nrr0: see there).  Returns the grid.  NOPRE = false: the caller never
// comes without a preconditioner (GraphOps::pcgIteration), and its translation unit does not instantiate ge_flatStepNoPre.
template <bool NOPRE, class T>
int launchFlatStep(const PcgIterArgs<T>& a, long nPad, int grid, bool lm, const LmStep<T>& L, const double* rr0, int nrr0, hipStream_t s) {
    if (a.pre)
        (lm ? ge_flatStep<T, true> : ge_flatStep<T, false>)<<<grid, kBlock, 0, s>>>(nPad, a.delta, a.pOld, a.rOld, a.ApOld, a.pre, a.rNew, a.pNew, a.aNumPrev.partials, a.aNumPrev.n,
            a.aDenPrev.partials, a.aDenPrev.n, a.s2Prev.partials, a.s2Prev.n, a.s3Prev.partials, a.s3Prev.n, L);
    else if constexpr (NOPRE)
        (lm ? ge_flatStepNoPre<T, true> : ge_flatStepNoPre<T, false>)<<<grid, kBlock, 0, s>>>(nPad, a.delta, a.pOld, a.rOld, a.ApOld, a.rNew, a.pNew, a.aNumPrev.partials, a.aNumPrev.n,
            a.aDenPrev.partials, a.aDenPrev.n, a.s2Prev.partials, a.s2Prev.n, a.s3Prev.partials, a.s3Prev.n, rr0, nrr0, L);
    return grid;
}
}  // namespace

}  // namespace optamd
