-- Spring mesh deformation: every mesh edge keeps its rest length, handles pull some vertices to targets.  NOT one of the energies built into libOpt.so:
-- its kernels live in the plug-in compiled from spring_mesh_deformation.hip (INTEGRATION.md, "Adding an energy without rebuilding libOpt.so").
-- problemparams layout:
--   [0] X            opt_float3[N]   unknown vertex positions
--   [1] UrShape      opt_float3[N]   rest positions
--   [2] Constraints  opt_float3[N]   handle targets; x < -999999.9 marks a free vertex
--   [3] w_fitSqrt, [4] w_regSqrt     float (host)
--   [5] G            int (host)      number of half-edges;  [6] v0, [7] v1: int[G]
local N = Dim("N", 0)
local X = Unknown("X", opt_float3, {N}, 0)
local UrShape = Image("UrShape", opt_float3, {N}, 1)
local Constraints = Image("Constraints", opt_float3, {N}, 2)
local w_fitSqrt = Param("w_fitSqrt", float, 3)
local w_regSqrt = Param("w_regSqrt", float, 4)
local G = Graph("G", 5, "v0", {N}, 6, "v1", {N}, 7)

UsePreconditioner(true)

-- handles
local pinned = greatereq(Constraints(0)(0), -999999.9)
Energy(Select(pinned, w_fitSqrt * (X(0) - Constraints(0)), 0))

-- an edge should keep the length it has in the rest shape
local function length(d) return Sqrt(Dot3(d, d)) end
Energy(w_regSqrt * (length(X(G.v1) - X(G.v0)) - length(UrShape(G.v1) - UrShape(G.v0))))
