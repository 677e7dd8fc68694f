// Type-erased view of the GN/LM solver that the C ABI (opt_api.cpp) drives.
#pragma once
#include "../../include/OptAmd.h"
#include "energy.h"

namespace optamd {

// reference solverGPUGaussNewton.t:148-163 (floats even in double mode), defaults :26-39
struct SolverParameters {
    float min_relative_decrease = 1e-3f;
    float min_trust_region_radius = 1e-32f;
    float max_trust_region_radius = 1e16f;
    float q_tolerance = 0.0001f;
    float function_tolerance = 0.000001f;
    float trust_region_radius = 1e4f;
    float radius_decrease_factor = 2.0f;
    float min_lm_diagonal = 1e-6f;
    float max_lm_diagonal = 1e32f;
    int residual_reset_period = 10;
    int nIter = 0;
    int nIterations = 10;
    int lIterations = 10;
    int patchIterations = 16;     // kind "patchGaussNewtonGPU" only: inner PCG iterations per patch and sweep (reference CUDAPatchSolverWarping.cpp:19)
    int patchSize = 32;           // 16 (the reference's PATCH_SIZE) or 32
    // Path selection (OptAmd.h "Solver parameters of this build"; reference callers never set them -- unknown names only warn there too, solver.t:1205-1221):
    int amd_reference_order = 0;  // 1: the reference's own sequence PCGStep1; PCGStep2; PCGStep3 per PCG iteration (solverGPUGaussNewton.t:1056-1092) on the generic kernels --
                                  // three sums per iteration as the reference forms them (r.z directly, no expansion; r, z, A p in memory).  The loop that meets the 1e-5 contract at
                                  // any horizon; ~3x the bytes of the default single-kernel iteration and never on chip.
    int amd_onchip = 1;           // 0: never take the on-chip (persistent) linear solve; 1: take it where the problem fits (default); 2: as 1, and the 5-point-stencil energies keep an LM solve on chip when a residual reset falls inside it; 3: as 2, and shape_from_shading too; 4: as 3, and image_warping takes the on-chip solve for any UrShape (not only the unit lattice); 5: as 4, and arap_mesh_deformation (volumetric_mesh_deformation too) runs the whole linear solve of a small symmetric graph in one workgroup; 6: as 5, and the functor mesh energies (cotangent, embedded, robust) run the whole linear solve of a small mesh in one workgroup too (graph_onchip.h); 7: as 6, and those energies may run it as one persistent launch of several workgroups (graph_onchip_grid.h; amd_onchip_workgroups)
    int amd_onchip_workgroups = 0;      // consulted at amd_onchip = 7 only (the functor mesh energies' linear solve as one persistent launch of several workgroups, graph_onchip_grid.h): 0 (default): the plan decides (GraphOps::ggAutoWorkgroups); n >= 1: n workgroups, clamped to one vertex per workgroup and to the family's cap of 32
    int amd_stencil_fused = 0;    // 1: the energies on the functor stencil engine (stencil_engine.h: optical_flow and intrinsic_image_decomposition wherever they run its launch-per-iteration loop, volumetric_mesh_deformation with OPT_AMD_VOLUMETRIC_ARAP=0, image-domain plug-ins) run two launches per PCG iteration (ge_flatStep + se_gatherIter); 0 (default): the reference's three.  Opt-in: the loop sums in another order and takes beta's numerator by expansion.  amd_reference_order = 1 wins; on-chip solves and the marching loops keep precedence; other energies ignore it
    int amd_graph_fused = 0;     // 1: cotangent_mesh_smoothing, embedded_mesh_deformation and robust_nonrigid_alignment run two launches per PCG iteration (ge_flatStep + ge_gather, graph_engine.h) and J^T J p without the per-(hyperedge, slot) records; 0 (default): the reference-order loop on the record kernels.  Opt-in: the fused loop sums in another order and takes beta's numerator by expansion.  amd_reference_order = 1 wins; other energies ignore it
};

struct SolverBase {
    SolverParameters sp;
    KernelTimer timer;
    int verbosity = 0;
    bool traceEnabled = false;
    bool insideSolve = false;    // set by Opt_ProblemSolve around its Init + Step loop: no caller code runs between those steps, so inputs other than the unknowns cannot change
    std::vector<double> trace;   // rows of 6
    virtual ~SolverBase() {}
    virtual void init(void** params) = 0;
    virtual int step(void** params) = 0;
    virtual double cost() const = 0;
    virtual long numUnknownScalars() const = 0;
    virtual void* vector(const std::string& name) = 0;
    virtual void evalJTF(void** params, void* jtf, void* diag) = 0;
    virtual double applyJTJ(void** params, const void* v, void* out) = 0;
    virtual double evalCost(void** params) = 0;
    virtual double trustRegionRadius() const = 0;
    virtual int onChipStatus() const { return 0; }             // OptAmd_PlanOnChipStatus
    virtual std::string describe() { return ""; }              // OptAmd_PlanDescribe
    virtual int setSlab(long row0, long rows, long globalHeight, const OptAmd_SlabComm* comm) = 0;
    virtual int setSlabExt(const OptAmd_SlabCommExt* ext) = 0;
    virtual void setTiming(int mode) = 0;                       // OptAmd_PlanSetTiming: 0 off, 1 an event pair per launch, 2 an event pair per run of launches of one name
    bool setParameter(const char* name, const void* value);   // solver.t:1205-1221
};

SolverBase* makeSolver(const EnergyInfo& info, bool lm, bool patch, bool doublePrecision, const unsigned* dims, bool timing, int verbosity);

}  // namespace optamd
