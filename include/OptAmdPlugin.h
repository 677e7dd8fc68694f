/* OptAmdPlugin.h -- energies that live outside libOpt.so.
 *
 * libOpt.so does not compile .t files: every energy it solves has a hand-written HIP kernel set, and twelve of them are built in.  A plug-in adds one
 * (or several) without rebuilding the library: a shared object that holds the energy's kernels and hands libOpt.so a registry entry per energy.
 * After OptAmd_LoadEnergyPlugin (OptAmd.h; or OPT_AMD_ENERGY_PLUGINS) the energy's .t file is planned, probed and solved through the unmodified Opt_* API.
 * This header is C++ (HIP): it is what a plug-in SOURCE includes, never what a caller of the library includes.
 * Such a source can be generated: opt_amd/tgen.py translates a .t of a documented subset of the DSL into one in the shape of the two worked examples (the functor,
 * its tables, the ParamDecls, the body hash), `python -m opt_amd.tgen my_energy.t` builds it.  What follows is the contract
 * such a source -- written or generated -- meets.
 *
 * A plug-in source for a MESH energy is (examples/plugins/spring_mesh_deformation.hip is the worked example; compile it with opt_amd/build.py build_plugin):
 *
 *     #pragma clang fp contract(off)          // (the engine's kernels expect the functor's arithmetic as written)
 *     #include "OptAmdPlugin.h"
 *     #include "graph_engine.h"               // the launch-per-iteration kernels: cost, J^T F, J^T J p, four or two launches per PCG iteration (amd_graph_fused)
 *     #include "graph_onchip.h"               // the whole linear solve in one workgroup (amd_onchip = 6)
 *     #include "graph_onchip_grid.h"          // ... in one launch of several workgroups (amd_onchip = 7)
 *     namespace optamd { namespace {          // (inside optamd: sqrt / sin / cos of a plain T are then the engine's overloads, as for its dual numbers)
 *     template <class T> struct MyG : GraphFunctorDefaults { ...the functor, see below... };
 *     EnergyInfo myInfo() {
 *         EnergyInfo e = graphEnergyInfo<MyG, true>("my_energy");      // UsePreconditioner(true); the .t file stem
 *         e.params = { ...one ParamDecl per declaration of the .t: kind, name, type, binding index... };
 *         e.bodyHashes = {0x...ul};           // OptAmd_ProblemFileHash of my_energy.t: the body these kernels implement
 *         return e;
 *     }
 *     } }
 *     OPTAMD_ENERGY_PLUGIN(optamd::myInfo)
 *
 * What a graph functor G provides (graph_engine.h instantiates every kernel from it; T is float or double):
 *   static constexpr int   NIMG            number of unknown images (Unknown(...) declarations over the vertex domain)
 *   static constexpr int   K               unknown scalars per vertex, all images together
 *   static constexpr int   V               vertices per hyperedge (slots of the Graph declaration)
 *   static constexpr int   RV, RE          scalar residuals per vertex (0 allowed) and per hyperedge
 *   static constexpr       imgOf(k), chOf(k), channels(img)      which image and channel unknown k of a vertex is; channels of an image  (__host__ __device__)
 *   static constexpr bool  edgeDepends(ri, j, k)    may edge residual ri depend on unknown k of slot j?  (true is always correct; false prunes derivative slots)
 *   static constexpr const char* kName     the name OptAmd_PlanDescribe prints in the kernel variant
 *   static int             unknownParam(img)        binding index of unknown image img
 *   members                long N; int nE; const int* vidx[V]; const T* X[NIMG];      vertex count (set by the engine), hyperedge count, index arrays, unknown images
 *   void bindParams(void** problemparams)  host: read every pointer and host scalar (Params are float on the host whatever T is; the edge count is an int)
 *   template <class S, class C> __device__ void vertexResiduals(const C& Xc, long v, S* r) const      r[0..RV): Xc(k) is unknown k of vertex v as an S
 *   template <class S, class C> __device__ void edgeResiduals(const C& Xc, long e, S* r) const        r[0..RE): Xc(j, k) is unknown k of slot j of hyperedge e
 * S is T or a dual number over T (stencil_engine.h Dual: + - * /, sqrt, sin, cos, valueOf): write the residuals once, with the .t's expressions; the engine
 * differentiates them.  A condition on a value takes valueOf(s).  Inputs that are not unknowns are read as plain T from the functor's own pointers.
 * The tuning constants of the on-chip solves come from GraphFunctorDefaults below unless the functor declares its own.
 *
 * A plug-in source for an IMAGE-DOMAIN energy (a 2-D or 3-D index space; examples/plugins/vector_tv_denoising.hip is the worked example) differs in its includes, its
 * functor and its registration call:
 *
 *     #include "OptAmdPlugin.h"
 *     #include "stencil_engine.h"             // cost, J^T F, J^T J p, model cost; three or two launches per PCG iteration (amd_stencil_fused)
 *     #include "graph_pcg.h"                  // ... whose flat pass (ge_flatStep) and host side live here (stencil_engine.h includes it; named for the reader)
 *     ... EnergyInfo e = stencilEnergyInfo<MyE, true>("my_energy"); ...
 *
 * What a stencil functor E provides (stencil_engine.h instantiates every kernel from it; T is float or double):
 *   static constexpr int   NDIM            dimensions of the index space (2 or 3; entries of `dimensions` consumed: W, H [, D])
 *   static constexpr int   NIMG            number of unknown images
 *   static constexpr int   K               unknown scalars per pixel, all images together
 *   static constexpr int   R               scalar residuals per pixel (every Energy(...) row, vector rows counted per channel, stencil rows per offset)
 *   static constexpr int   NOFF            stencil offsets at which a residual reads an UNKNOWN, the centre included
 *   static constexpr int   NAUX            planes of ComputedArrays (0: none); with NAUX > 0 the engine owns `aux` (plane k at aux + k W H D) and fills it
 *                                          with computeAux after bind and after every update or revert
 *   static constexpr       off(i, axis)    offset i along axis 0 / 1 / 2 (x / y / z); off(0, .) == 0: offset 0 is the centre  (__host__ __device__)
 *   static constexpr       imgOf(k), chOf(k), channels(img)      which image and channel unknown k of a pixel is; channels of an image  (__host__ __device__)
 *   static constexpr bool  depends(ri, oi) may residual ri depend on the unknowns at offset oi?  (true is always correct; false prunes derivative work)
 *   static constexpr const char* kName     the name OptAmd_PlanDescribe prints in the kernel variant
 *   static int             unknownParam(img)        binding index of unknown image img
 *   members                int W, H, D; const T* X[NIMG]; T* aux;      the index space (set by the engine; 1 beyond NDIM), the unknown images, the aux planes
 *   void bindParams(void** problemparams)  host: read every pointer and host scalar (Params are float on the host whatever T is)
 *   __device__ bool excluded(int x, int y, int z) const          restates the .t's Exclude(...): the pixel is not an unknown (its rows of J^T F, diag and
 *                                          J^T J p are 0, the residuals centred on it do not count in the cost but do count for its neighbours)
 *   __device__ void computeAux(int x, int y, int z, T* out) const      out[0..NAUX): the ComputedArrays at the pixel, from the current unknowns
 *   template <class S, class C> __device__ void residuals(const C& Xc, int x, int y, int z, S* r) const      r[0..R) of the residuals CENTRED at (x, y, z):
 *                                          Xc(k, dx, dy, dz) is unknown k at that offset from the centre as an S (0 outside the image, like the reference's
 *                                          image loads), Xc.in(dx, dy, dz) says whether the offset is inside the image
 * A residual whose stencil leaves the image is the functor's business: it must restate the InBounds / default-zero rule of its .t (typically
 * r[i] = Xc.in(dx, dy, 0) ? e : S(T(0))).  Every offset passed to Xc must be one of off(i, .).  S is T or a dual number over T, as for graph functors; the helpers
 * are valueOf(s) (the plain value, for conditions and for sampling positions), chain1(f, f', u) and chain2(f, fu, fv, u, v) (a function of one or two unknowns
 * whose value and partials are known: a table, a sampled image).  StencilFunctorDefaults<T> below supplies NAUX = 0, aux, an empty computeAux and
 * excluded() == false for a functor that needs none of them.
 * Image-domain plug-ins run the engine's launch-per-iteration loops only.  The marching Gauss-Newton loop (stencil_march.h) and the on-chip stencil solves
 * (stencil_onchip.h) need a hand-written 5-point operator besides the functor and are not offered to plug-in sources.
 *
 * The .t and the hash rule.  The .t file is what the caller passes to Opt_ProblemDefine, written as the reference would accept it; libOpt.so reads its
 * declarations (they must match `params`: kind, name, type, binding index; and UsePreconditioner) and hashes its body.  Only a body whose hash the entry
 * records is accepted -- the kernels are what is solved, so an edited Energy line must come with edited kernels and a new hash.  An entry without a hash
 * is refused: for plug-ins there is no unchecked mode.
 *
 * The ABI stamp rule.  libOpt.so calls the plug-in's kernel set through the C++ types of opt_amd/csrc/energy.h.  Both sides compute a stamp from
 * kEnergyAbiVersion and the sizes of those types as they compiled them; the loader asks for the stamp first and runs nothing else of a plug-in whose stamp
 * differs.  Rebuild plug-ins together with the library.  Whoever changes EnergyOps, EnergyInfo, ParamDecl, LaunchCtx, Reduction, KernelTimer or OnchipGuard
 * bumps kEnergyAbiVersion.
 *
 * No unloading.  A loaded plug-in stays mapped until the process ends (no dlclose): plans hold objects whose code lives in it, and the HIP runtime has
 * registered its kernels.
 */
#pragma once
#include "../opt_amd/csrc/energy.h"
#include "../opt_amd/csrc/onchip_sync.h"

namespace optamd {

/* The stamp of the kernel-set interface as THIS translation unit compiled it. */
constexpr unsigned long energyAbiStamp(unsigned version) {
    unsigned long h = 0xcbf29ce484222325ul;
    const unsigned long parts[] = {version, sizeof(EnergyOps<float>), sizeof(EnergyOps<double>), sizeof(EnergyInfo), sizeof(ParamDecl), sizeof(LaunchCtx),
                                   sizeof(Reduction), sizeof(KernelTimer), sizeof(OnchipGuard), sizeof(PcgIterArgs<double>), sizeof(LmInitArgs<double>), sizeof(OnChipLm<double>)};
    for (unsigned long p : parts) { h ^= p; h *= 0x100000001b3ul; }
    return h;
}
/* -DOPTAMD_PLUGIN_ABI_SKEW=n builds a plug-in that reports the stamp of another interface version: the loader's refusal is tested with it, nothing else uses it. */
#ifndef OPTAMD_PLUGIN_ABI_SKEW
#define OPTAMD_PLUGIN_ABI_SKEW 0
#endif
constexpr unsigned long kEnergyAbiStamp = energyAbiStamp(kEnergyAbiVersion + OPTAMD_PLUGIN_ABI_SKEW);

/* The one symbol a plug-in exports (OPTAMD_ENERGY_PLUGIN defines it).  Always writes the plug-in's stamp to *stamp.  sink == nullptr: nothing else (the loader's
 * first call).  Otherwise appends the plug-in's entries to *sink and returns their number. */
#define OPTAMD_PLUGIN_ENTRY_NAME "OptAmdPlugin_Energies"
typedef int (*EnergyPluginEntry)(unsigned long* stamp, std::vector<EnergyInfo>* sink);

/* Conservative tuning constants of the on-chip solves (graph_onchip.h, graph_onchip_grid.h), indexed [float, double] ([..][GN, LM] for kOnChipV).  A functor that
 * derives from this and declares none of them gets: one vertex per lane in the one-workgroup solve (meshes up to 512 vertices), two slots differentiated per pass,
 * p and delta in LDS (r and A p in registers), and no automatic workgroup count at amd_onchip = 7 -- several workgroups only where the caller sets
 * amd_onchip_workgroups, level 6's behaviour otherwise.  Every variant is still subject to the engine's run-time gate: one that needs scratch memory is not offered.
 * Redeclare a constant in the functor to override it; profiles/onchip_graph.md and profiles/onchip_graph_grid.md show how the built-in functors' values were measured. */
struct GraphFunctorDefaults {
    static constexpr int kOnChipV[2][2] = {{1, 1}, {1, 1}};
    static constexpr int kOnChipSlotsPerPass[2] = {2, 2};
    static constexpr int kOnChipLdsVectors[2] = {2, 2};
    static constexpr long kOnChipGridAutoMaxVertices[2] = {0, 0};
    static constexpr bool kSlotAtRunTime = true;      /* one body per hyperedge evaluation with the slot chosen at run time (false: V compile-time bodies) */
};

/* The registry entry of a mesh energy over one index space, served by the graph engine instantiated for the functor template G: name (the .t file stem), the
 * factories for float and double, UsePreconditioner.  `params` and `bodyHashes` are the author's to fill in.  (The source includes graph_engine.h, graph_onchip.h
 * and graph_onchip_grid.h before it calls this.) */
template <class T, class G> struct GraphOps;
template <template <class> class G, bool USE_PRECONDITIONER, class T>
EnergyOps<T>* makeGraphOps(const unsigned* dims) { return new GraphOps<T, G<T>>(dims, USE_PRECONDITIONER); }
template <template <class> class G, bool USE_PRECONDITIONER>
EnergyInfo graphEnergyInfo(const char* name) {
    EnergyInfo e;
    e.name = name; e.nDims = 1; e.usePreconditioner = USE_PRECONDITIONER; e.floatOnly = false;
    e.residualsPerElement = G<float>::RV; e.residualsPerEdge = G<float>::RE;
    e.makeFloat = makeGraphOps<G, USE_PRECONDITIONER, float>; e.makeDouble = makeGraphOps<G, USE_PRECONDITIONER, double>;
    return e;
}

/* What a stencil functor that has no ComputedArrays and excludes nothing need not write itself (redeclare a member in the functor to override it). */
template <class T>
struct StencilFunctorDefaults {
    static constexpr int NAUX = 0;
    T* aux;
    __device__ void computeAux(int, int, int, T*) const {}
    __device__ bool excluded(int, int, int) const { return false; }
};

/* The registry entry of an image-domain energy over one 2-D or 3-D index space, served by the stencil engine instantiated for the functor template E.  `params` and
 * `bodyHashes` are the author's to fill in.  (The source includes stencil_engine.h before it calls this.) */
template <class T, class E> struct StencilOps;
template <template <class> class E, bool USE_PRECONDITIONER, class T>
EnergyOps<T>* makeStencilOps(const unsigned* dims) { return new StencilOps<T, E<T>>(dims, USE_PRECONDITIONER); }
template <template <class> class E, bool USE_PRECONDITIONER>
EnergyInfo stencilEnergyInfo(const char* name) {
    EnergyInfo e;
    e.name = name; e.nDims = E<float>::NDIM; e.usePreconditioner = USE_PRECONDITIONER; e.floatOnly = false;
    e.residualsPerElement = E<float>::R;
    e.makeFloat = makeStencilOps<E, USE_PRECONDITIONER, float>; e.makeDouble = makeStencilOps<E, USE_PRECONDITIONER, double>;
    return e;
}

}  // namespace optamd

/* Defines the plug-in's entry from functions that return an EnergyInfo each:  OPTAMD_ENERGY_PLUGIN(myInfo)  or  OPTAMD_ENERGY_PLUGIN(infoA, infoB). */
#define OPTAMD_ENERGY_PLUGIN(...)                                                                                                       \
    extern "C" __attribute__((visibility("default"))) int OptAmdPlugin_Energies(unsigned long* stamp, std::vector<optamd::EnergyInfo>* sink) { \
        *stamp = optamd::kEnergyAbiStamp;                                                                                               \
        if (!sink) return 0;                                                                                                            \
        optamd::EnergyInfo (*const fns[])() = {__VA_ARGS__};                                                                            \
        for (auto fn : fns) sink->push_back(fn());                                                                                      \
        return (int)(sizeof(fns) / sizeof(fns[0]));                                                                                     \
    }
