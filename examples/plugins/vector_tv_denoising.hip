// An image-domain energy plug-in (include/OptAmdPlugin.h): vector_tv_denoising.t served by the functor stencil engine, compiled into a library of its own and loaded
// into libOpt.so at run time (OptAmd_LoadEnergyPlugin / OPT_AMD_ENERGY_PLUGINS).  Build: opt_amd/build.py build_plugin("examples/plugins/vector_tv_denoising.hip").
// A source like this one is all a new image energy needs: the functor, the declarations of its .t, the body hash, one registration line.
// No fused multiply-adds: the cost pass (S = T) and the derivative passes (S = dual numbers) must form the same residual bits.
#pragma clang fp contract(off)
#include "OptAmdPlugin.h"
#include "stencil_engine.h"      // cost, J^T F, J^T J p, model cost; three launches per PCG iteration, two with amd_stencil_fused = 1
#include "graph_pcg.h"           // (the flat pass of the two-launch iteration; stencil_engine.h includes it)

namespace optamd {      // (the functor's sqrt on S = T is the engine's overload, found here)
namespace {

// vector_tv_denoising.t.  X float2 per pixel; fit w_fitSqrt (X - A) per channel; for the forward neighbours n = (1,0), (0,1), where in bounds,
// w_regSqrt (sqrt(|X(0,0) - X(n)|^2 + eps^2) - eps).  Exclude(Mask > 0).  UsePreconditioner(true).  No ComputedArrays: StencilFunctorDefaults.
template <class T>
struct VectorTvE : StencilFunctorDefaults<T> {
    static constexpr const char* kName = "VectorTvE";
    static constexpr int NDIM = 2, NIMG = 1, K = 2, R = 4, NOFF = 3;
    static constexpr __host__ __device__ int off(int i, int a) { return a == 0 ? (i == 1 ? 1 : 0) : a == 1 ? (i == 2 ? 1 : 0) : 0; }      // centre, (1,0), (0,1)
    static constexpr __host__ __device__ int imgOf(int) { return 0; }
    static constexpr __host__ __device__ int chOf(int k) { return k; }
    static constexpr __host__ __device__ int channels(int) { return 2; }
    // rows 0, 1: fit (centre only); row 2: the difference to (1,0); row 3: to (0,1)
    static constexpr __host__ __device__ bool depends(int ri, int oi) { return oi == 0 || (ri >= 2 && ri - 1 == oi); }
    static int unknownParam(int) { return 0; }
    int W, H, D;
    const T* X[NIMG];
    const T *A, *Mask; T w_fit, w_reg, eps;
    void bindParams(void** p) {
        X[0] = (const T*)p[0]; A = (const T*)p[1]; Mask = (const T*)p[2];
        w_fit = (T) * (const float*)p[3]; w_reg = (T) * (const float*)p[4]; eps = (T) * (const float*)p[5];
    }
    __device__ bool excluded(int x, int y, int) const { return Mask[(long)y * W + x] > T(0); }      // Exclude(greater(Mask(0,0), 0))
    template <class S, class C>
    __device__ __forceinline__ void residuals(const C& Xc, int x, int y, int, S* r) const {
        const long i = (long)y * W + x;
        const S u = Xc(0), v = Xc(1);
        r[0] = w_fit * (u - A[2 * i]); r[1] = w_fit * (v - A[2 * i + 1]);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int dx = off(n + 1, 0), dy = off(n + 1, 1);
            const S du = u - Xc(0, dx, dy), dv = v - Xc(1, dx, dy);
            const S e = w_reg * (sqrt(du * du + dv * dv + eps * eps) - eps);
            r[2 + n] = Xc.in(dx, dy, 0) ? e : S(T(0));      // Select(InBounds(dx,dy), ., 0)
        }
    }
};

EnergyInfo vectorTvInfo() {
    EnergyInfo e = stencilEnergyInfo<VectorTvE, true>("vector_tv_denoising");
    e.params = {{ParamDecl::kUnknown, "X", "opt_float2", 0}, {ParamDecl::kArray, "A", "opt_float2", 1}, {ParamDecl::kArray, "Mask", "opt_float", 2},
                {ParamDecl::kScalar, "w_fitSqrt", "float", 3}, {ParamDecl::kScalar, "w_regSqrt", "float", 4}, {ParamDecl::kScalar, "eps", "float", 5}};
    e.bodyHashes = {0xfabadde5f39508cbul};     // OptAmd_ProblemFileHash("vector_tv_denoising.t")
    return e;
}

}  // namespace
}  // namespace optamd

OPTAMD_ENERGY_PLUGIN(optamd::vectorTvInfo)
