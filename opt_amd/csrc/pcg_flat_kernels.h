// The flat streaming kernels of the PCG solver (solver.hip): 16-byte packs over the FLAT unknown vector, per-workgroup partial sums in double.
#pragma once
#include "common.h"

namespace optamd {

// ------------------------------------------------------------------------------------------------------
// 16-byte packs of opt_float
template <class T> struct Pack;
template <> struct alignas(16) Pack<float> { float v[4]; };
template <> struct alignas(16) Pack<double> { double v[2]; };
template <class T> struct PackN;
template <> struct PackN<float> { static constexpr int N = 4; typedef float vec __attribute__((ext_vector_type(4))); };
template <> struct PackN<double> { static constexpr int N = 2; typedef double vec __attribute__((ext_vector_type(2))); };

// Streaming (non-temporal) 16-byte accesses: every PCG vector is far larger than L2 + Infinity Cache and is
// touched once per kernel, so the hot streaming kernels ask the memory system not to retain the lines.
// Measured on MI355X (tools/microbench_stream.hip, PCGStep2 shape at 4096^2): plain 302 us, nt + 2 packs in
// flight per lane 270 us.
#ifndef S2_NT_LOAD
#define S2_NT_LOAD 1
#endif
template <class T> __device__ __forceinline__ Pack<T> ldnt(const T* base, long i) {
    typedef typename PackN<T>::vec V;
    const V v = S2_NT_LOAD ? __builtin_nontemporal_load((const V*)base + i) : ((const V*)base)[i];
    Pack<T> p;
#pragma unroll
    for (int k = 0; k < PackN<T>::N; ++k) p.v[k] = v[k];
    return p;
}
template <class T> __device__ __forceinline__ void stnt(T* base, long i, const Pack<T>& p) {
    typedef typename PackN<T>::vec V;
    V v;
#pragma unroll
    for (int k = 0; k < PackN<T>::N; ++k) v[k] = p.v[k];
    __builtin_nontemporal_store(v, (V*)base + i);
}

template <class T> __device__ __forceinline__ T guardedInvert(T x) {   // solver.t:323-332 (CERES)
    T s = T(1) + sqrt(x);
    return T(1) / (s * s);
}

// PCGInit1 (non-graph tail) / PCGInit1_Finish (graph): solver.t:384-392, 399-419.  r already holds -J^T F.
template <class T>
__global__ __launch_bounds__(kBlock) void k_initFinish(const T* __restrict__ r, const T* __restrict__ diag, T* __restrict__ pre,
                                                       T* __restrict__ p, T* __restrict__ delta, long nPacks, int usePre, int graphMode,
                                                       double* __restrict__ partials) {
    __shared__ double scratch[kBlock / kWave + 1];
    constexpr int N = PackN<T>::N;
    double acc = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nPacks; i += (long)gridDim.x * blockDim.x) {
        Pack<T> R = ((const Pack<T>*)r)[i], D = ((const Pack<T>*)diag)[i], PR, PP, Z;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            T d = usePre ? D.v[k] : T(1);
            T pr = guardedInvert(d);
            if (graphMode && !usePre) pr = T(1);
            T pp = pr * R.v[k];
            PR.v[k] = pr; PP.v[k] = pp; Z.v[k] = T(0);
            acc += (double)(R.v[k] * pp);
        }
        ((Pack<T>*)pre)[i] = PR; ((Pack<T>*)p)[i] = PP; ((Pack<T>*)delta)[i] = Z;
    }
    double t = blockReduceSum(acc, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// total[0] = sum(partials[0..n))   (one workgroup)
__global__ __launch_bounds__(kBlock) void k_finalizeSum(const double* __restrict__ partials, int n, double* __restrict__ total) {
    __shared__ double scratch[kBlock / kWave + 1];
    double s = sumPartials(partials, n, scratch);
    if (threadIdx.x == 0) total[0] = s;
}

// total[k] = sum(partials_k[0..n_k)) for four reductions at once: workgroup k handles array k (slab mode: one launch
// before the single 4-double all-reduce of the fused PCG iteration)
struct Partials4 { const double* p[4]; int n[4]; };
__global__ __launch_bounds__(kBlock) void k_finalizeSum4(Partials4 in, double* __restrict__ total) {
    __shared__ double scratch[kBlock / kWave + 1];
    double s = sumPartials(in.p[blockIdx.x], in.n[blockIdx.x], scratch);
    if (threadIdx.x == 0) total[blockIdx.x] = s;
}

// PCGStep2: solver.t:446-489
template <class T, bool LM>
__global__ __launch_bounds__(kBlock) void k_step2(T* __restrict__ delta, const T* __restrict__ p, T* __restrict__ r, const T* __restrict__ Ap,
                                                  const T* __restrict__ pre /*nullptr -> 1*/, const T* __restrict__ b, T* __restrict__ z, long nPacks,
                                                  const double* __restrict__ aNumTotal, const double* __restrict__ aDenPartials, int nDen,
                                                  double* __restrict__ bNumPartials, double* __restrict__ qPartials) {
    __shared__ double scratch[kBlock / kWave + 1];
    constexpr int N = PackN<T>::N;
    const T aDen = (T)sumPartials(aDenPartials, nDen, scratch);
    const T aNum = (T)aNumTotal[0];
    const T alpha = (aDen > T(0)) ? aNum / aDen : T(0);   // guardDivisionByZero, solver.t:456-459
    double accB = 0, accQ = 0;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x; i0 < nPacks; i0 += 2 * stride) {
        // two packs per lane in flight: issue all loads of both before the first use
        Pack<T> D[2], P[2], R[2], A[2], M[2], B[2], Z;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long i = i0 + u * stride;
            if (i < nPacks) {
                D[u] = ldnt(delta, i); P[u] = ldnt(p, i); R[u] = ldnt(r, i); A[u] = ldnt(Ap, i);
                if (pre) M[u] = ldnt(pre, i);
                if (LM) B[u] = ldnt(b, i);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long i = i0 + u * stride;
            if (i < nPacks) {
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    T dl = D[u].v[k] + alpha * P[u].v[k];
                    T rr = R[u].v[k] - alpha * A[u].v[k];
                    T m = pre ? M[u].v[k] : T(1);
                    T zz = m * rr;
                    D[u].v[k] = dl; R[u].v[k] = rr; Z.v[k] = zz;
                    accB += (double)(zz * rr);
                    if (LM) accQ += (double)(T(0.5) * (dl * (rr + B[u].v[k])));
                }
                stnt(delta, i, D[u]); stnt(r, i, R[u]); stnt(z, i, Z);      // non-temporal: nothing of this pass is read again before the next one has streamed past it
            }
        }
    }
    double t = blockReduceSum(accB, scratch);
    if (threadIdx.x == 0) bNumPartials[blockIdx.x] = t;
    if (LM) {
        double tq = blockReduceSum(accQ, scratch);
        if (threadIdx.x == 0) qPartials[blockIdx.x] = tq;
    }
}

// PCGStep2_1stHalf: solver.t:491-503
// deltaOut may be delta (in place) or another vector (the caller then decides later which of the two it keeps).  alphaNumerator is either a
// finished total (aNumTotal, nNum == 0) or partial sums this kernel adds up itself -- the same sumPartials over kBlock threads as
// k_finalizeSum, so the same bits, one launch less.
// pOwed / alphaOwed (may be null): a term alphaOwed[0] * pOwed that an earlier launch left owed to delta (PcgIterResult::owedP) is added first -- the reference's
// order of additions, one pass instead of two.
template <class T>
__global__ __launch_bounds__(kBlock) void k_step2FirstHalf(const T* delta, T* deltaOut, const T* __restrict__ p, long nPacks, const double* __restrict__ aNumTotal,
                                                           const double* __restrict__ aNumPartials, int nNum, const double* __restrict__ aDenPartials, int nDen,
                                                           const T* __restrict__ pOwed = nullptr, const T* __restrict__ alphaOwed = nullptr) {
    __shared__ double scratch[kBlock / kWave + 1];
    constexpr int N = PackN<T>::N;
    const T aDen = (T)sumPartials(aDenPartials, nDen, scratch);
    const T aNum = nNum > 0 ? (T)sumPartials(aNumPartials, nNum, scratch) : (T)aNumTotal[0];
    const T alpha = (aDen > T(0)) ? aNum / aDen : T(0);
    const T a2 = pOwed ? alphaOwed[0] : T(0);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nPacks; i += (long)gridDim.x * blockDim.x) {
        Pack<T> D = ((const Pack<T>*)delta)[i], P = ((const Pack<T>*)p)[i];
        if (pOwed) {
            const Pack<T> P2 = ((const Pack<T>*)pOwed)[i];
#pragma unroll
            for (int k = 0; k < N; ++k) D.v[k] = D.v[k] + a2 * P2.v[k];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) D.v[k] = D.v[k] + alpha * P.v[k];
        ((Pack<T>*)deltaOut)[i] = D;
    }
}

// Completion stamp for PcgSolver::drain(): everything enqueued before it has finished when the host sees the value.
__global__ void k_stamp(unsigned long long* flag, unsigned long long v) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// PCGStep2_2ndHalf: solver.t:505-534
template <class T>
__global__ __launch_bounds__(kBlock) void k_step2SecondHalf(const T* __restrict__ delta, T* __restrict__ r, const T* __restrict__ Adelta, const T* __restrict__ b,
                                                            const T* __restrict__ pre, T* __restrict__ z, long nPacks, double* __restrict__ bNumPartials,
                                                            double* __restrict__ qPartials) {
    __shared__ double scratch[kBlock / kWave + 1];
    constexpr int N = PackN<T>::N;
    double accB = 0, accQ = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nPacks; i += (long)gridDim.x * blockDim.x) {
        Pack<T> D = ((const Pack<T>*)delta)[i], A = ((const Pack<T>*)Adelta)[i], B = ((const Pack<T>*)b)[i], M, R, Z;
        if (pre) M = ((const Pack<T>*)pre)[i];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            T rr = B.v[k] - A.v[k];
            T m = pre ? M.v[k] : T(1);
            T zz = m * rr;
            R.v[k] = rr; Z.v[k] = zz;
            accB += (double)(zz * rr);
            accQ += (double)(T(0.5) * (D.v[k] * (rr + B.v[k])));
        }
        ((Pack<T>*)r)[i] = R; ((Pack<T>*)z)[i] = Z;
    }
    double t = blockReduceSum(accB, scratch);
    if (threadIdx.x == 0) bNumPartials[blockIdx.x] = t;
    double tq = blockReduceSum(accQ, scratch);
    if (threadIdx.x == 0) qPartials[blockIdx.x] = tq;
}

// PCGStep3: solver.t:537-550; workgroup 0 also publishes betaNumerator as the next alphaNumerator (:1091)
template <class T>
__global__ __launch_bounds__(kBlock) void k_step3(const T* __restrict__ z, T* __restrict__ p, long nPacks, const double* __restrict__ bNumPartials, int nB,
                                                  const double* __restrict__ aNumOld, double* __restrict__ aNumNext) {
    __shared__ double scratch[kBlock / kWave + 1];
    constexpr int N = PackN<T>::N;
    const double bSum = sumPartials(bNumPartials, nB, scratch);
    const T rDotzNew = (T)bSum, rDotzOld = (T)aNumOld[0];
    const T beta = (rDotzOld > T(0)) ? rDotzNew / rDotzOld : T(0);
    if (blockIdx.x == 0 && threadIdx.x == 0) aNumNext[0] = bSum;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nPacks; i += (long)gridDim.x * blockDim.x) {
        Pack<T> Z = ((const Pack<T>*)z)[i], P = ((Pack<T>*)p)[i];
#pragma unroll
        for (int k = 0; k < N; ++k) P.v[k] = Z.v[k] + beta * P.v[k];
        ((Pack<T>*)p)[i] = P;
    }
}

// PCGLinearUpdate / revertUpdate / savePreviousUnknowns on one unknown image (caller-owned array, not padded)
template <class T>
__global__ __launch_bounds__(kBlock) void k_axpyImage(T* __restrict__ X, const T* __restrict__ d, long n) {   // X += d   (solver.t:552-557)
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) X[i] = X[i] + d[i];
}
template <class T>
__global__ __launch_bounds__(kBlock) void k_saveAndUpdate(T* __restrict__ X, T* __restrict__ prev, const T* __restrict__ d, long n) {   // prev = X; X += d  (LM: solver.t:1113-1114 in one pass)
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) { const T x = X[i]; prev[i] = x; X[i] = x + d[i]; }
}
template <class T>
__global__ __launch_bounds__(kBlock) void k_copy(T* __restrict__ dst, const T* __restrict__ src, long n) {    // solver.t:559-564, 573-578, 624-629
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = src[i];
}

// PCGComputeCtC + PCGFinalizeDiagonal: solver.t:616-622, 631-664.  On entry CtC holds raw diag(J^T J).
// INIT: the kernel also does what PCGInit1's tail does in an LM step before it (k_initFinish: delta = 0, the guarded-inverse preconditioner -- needed only to
// seed SSq at the first outer iteration, solver.t:635 -- and a p that this kernel overwrites anyway): one pass over the vectors instead of two or three.
template <class T, bool INIT>
__global__ __launch_bounds__(kBlock) void k_finalizeDiagonal(T* __restrict__ CtC, T* __restrict__ SSq, const T* __restrict__ r, T* __restrict__ delta,
                                                             T* __restrict__ pre, T* __restrict__ b, T* __restrict__ p, long nPacks, T radius, T minLm, T maxLm,
                                                             double* __restrict__ dPartials, double* __restrict__ qPartials, int usePre, int graphMode, int saveSSq) {
    __shared__ double scratch[kBlock / kWave + 1];
    constexpr int N = PackN<T>::N;
    const T invRadius = T(1) / radius;
    double accD = 0, accQ = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nPacks; i += (long)gridDim.x * blockDim.x) {
        Pack<T> C = ((Pack<T>*)CtC)[i], R = ((const Pack<T>*)r)[i], S, D, M, P;
        if (INIT) {
#pragma unroll
            for (int k = 0; k < N; ++k) {
                T pr = guardedInvert(usePre ? C.v[k] : T(1));      // k_initFinish
                if (graphMode && !usePre) pr = T(1);
                S.v[k] = pr; D.v[k] = T(0);
            }
            if (saveSSq) ((Pack<T>*)SSq)[i] = S;                   // PCGSaveSSq (first outer iteration)
            else S = ((const Pack<T>*)SSq)[i];
            ((Pack<T>*)delta)[i] = D;
        } else { S = ((const Pack<T>*)SSq)[i]; D = ((const Pack<T>*)delta)[i]; }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            T unclamped = C.v[k] * invRadius;                 // computeCtC: diag(J^T J) / radius (o.t:2277-2279)
            T invS = T(1) / S.v[k];
            T clampMul = invS / radius;
            T lo = minLm * clampMul, hi = maxLm * clampMul;
            T c = fmin(fmax(unclamped, lo), hi);
            C.v[k] = c;
            T m = T(1) / (c + radius * unclamped);
            M.v[k] = m;
            T pp = m * R.v[k];
            P.v[k] = pp;
            accD += (double)(R.v[k] * pp);
            accQ += (double)(T(0.5) * (D.v[k] * (R.v[k] + R.v[k])));
        }
        ((Pack<T>*)CtC)[i] = C; ((Pack<T>*)pre)[i] = M; ((Pack<T>*)b)[i] = R; ((Pack<T>*)p)[i] = P;
    }
    double t = blockReduceSum(accD, scratch);
    if (threadIdx.x == 0) dPartials[blockIdx.x] = t;
    double tq = blockReduceSum(accQ, scratch);
    if (threadIdx.x == 0) qPartials[blockIdx.x] = tq;
}

}  // namespace optamd
