// An energy plug-in (include/OptAmdPlugin.h): spring_mesh_deformation.t served by the graph functor engine, compiled into a library of its own and loaded into
// libOpt.so at run time (OptAmd_LoadEnergyPlugin / OPT_AMD_ENERGY_PLUGINS).  Build: opt_amd/build.py build_plugin("examples/plugins/spring_mesh_deformation.hip").
// A source like this one is all a new mesh energy needs: the functor, the declarations of its .t, the body hash, one registration line.
// No fused multiply-adds: the cost pass (S = T) and the derivative passes (S = dual numbers) must form the same residual bits.
#pragma clang fp contract(off)
#include "OptAmdPlugin.h"
#include "graph_engine.h"
#include "graph_onchip.h"      // the whole linear solve of a small mesh in one workgroup (amd_onchip = 6)
#include "graph_onchip_grid.h" // ... and of a larger one as one launch of several workgroups (amd_onchip = 7, amd_onchip_workgroups)

namespace optamd {      // (the functor's sqrt / sin / cos on S = T are the engine's overloads, found here)
namespace {

// spring_mesh_deformation.t.  X float3 per vertex; fit w_fitSqrt (X - Constraints) where Constraints.x >= -999999.9; per half-edge
// w_regSqrt (|X_v1 - X_v0| - |UrShape_v1 - UrShape_v0|).  UsePreconditioner(true).  The tuning constants of the on-chip solves are GraphFunctorDefaults'.
template <class T>
struct SpringG : GraphFunctorDefaults {
    static constexpr const char* kName = "SpringG";
    static constexpr int NIMG = 1, K = 3, V = 2, RV = 3, RE = 1;
    static constexpr __host__ __device__ int imgOf(int) { return 0; }
    static constexpr __host__ __device__ int chOf(int k) { return k; }
    static constexpr __host__ __device__ int channels(int) { return 3; }
    static constexpr __host__ __device__ bool edgeDepends(int, int, int) { return true; }      // the length couples the three components of both vertices
    static int unknownParam(int) { return 0; }
    long N; int nE; const int* vidx[V]; const T* X[NIMG];
    const T *Ur, *Cons; T w_fit, w_reg;
    void bindParams(void** p) {
        X[0] = (const T*)p[0]; Ur = (const T*)p[1]; Cons = (const T*)p[2];
        w_fit = (T) * (const float*)p[3]; w_reg = (T) * (const float*)p[4];
        nE = *(const int*)p[5]; vidx[0] = (const int*)p[6]; vidx[1] = (const int*)p[7];      // Graph("G", 5, "v0", {N}, 6, "v1", {N}, 7)
    }
    template <class S, class C> __device__ __forceinline__ void vertexResiduals(const C& Xc, long v, S* r) const {
        const bool valid = Cons[3 * v] >= T(-999999.9);
#pragma unroll
        for (int c = 0; c < 3; ++c) { const S e = w_fit * (Xc(c) - Cons[3 * v + c]); r[c] = valid ? e : S(T(0)); }
    }
    template <class S, class C> __device__ __forceinline__ void edgeResiduals(const C& Xc, long e, S* r) const {
        const long a = vidx[0][e], b = vidx[1][e];
        const T u[3] = {Ur[3 * b] - Ur[3 * a], Ur[3 * b + 1] - Ur[3 * a + 1], Ur[3 * b + 2] - Ur[3 * a + 2]};
        const S d[3] = {Xc(1, 0) - Xc(0, 0), Xc(1, 1) - Xc(0, 1), Xc(1, 2) - Xc(0, 2)};
        const S len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        r[0] = w_reg * (len - sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]));
    }
};

EnergyInfo springInfo() {
    EnergyInfo e = graphEnergyInfo<SpringG, true>("spring_mesh_deformation");
    e.params = {{ParamDecl::kUnknown, "X", "opt_float3", 0}, {ParamDecl::kArray, "UrShape", "opt_float3", 1}, {ParamDecl::kArray, "Constraints", "opt_float3", 2},
                {ParamDecl::kScalar, "w_fitSqrt", "float", 3}, {ParamDecl::kScalar, "w_regSqrt", "float", 4},
                {ParamDecl::kGraphCount, "G", "int", 5}, {ParamDecl::kGraphIndex, "G.v0", "int", 6}, {ParamDecl::kGraphIndex, "G.v1", "int", 7}};
    e.bodyHashes = {0x2b632b6a46af6c0bul};     // OptAmd_ProblemFileHash("spring_mesh_deformation.t")
    return e;
}

}  // namespace
}  // namespace optamd

OPTAMD_ENERGY_PLUGIN(optamd::springInfo)
