-- Vector total-variation denoising: a two-channel field X stays near its noisy observation A while the smoothed length of its forward
-- differences is penalised (the two channels share one length: they are coupled).  NOT one of the energies built into libOpt.so: its kernels live
-- in the plug-in compiled from vector_tv_denoising.hip (INTEGRATION.md, "Adding an energy without rebuilding libOpt.so", the image-domain example).
-- problemparams layout:
--   [0] X      opt_float2[W*H]   unknown field
--   [1] A      opt_float2[W*H]   noisy observation
--   [2] Mask   opt_float [W*H]   > 0: the pixel is not an unknown (it keeps its value and still bounds its neighbours' differences)
--   [3] w_fitSqrt, [4] w_regSqrt, [5] eps   float (host); eps > 0 smooths the length at zero
local W, H = Dim("W", 0), Dim("H", 1)
local X = Unknown("X", opt_float2, {W,H}, 0)
local A = Array("A", opt_float2, {W,H}, 1)
local Mask = Array("Mask", opt_float, {W,H}, 2)
local w_fitSqrt = Param("w_fitSqrt", float, 3)
local w_regSqrt = Param("w_regSqrt", float, 4)
local eps = Param("eps", float, 5)

UsePreconditioner(true)
Exclude(greater(Mask(0,0), 0))

-- data term, one residual per channel
Energy(w_fitSqrt * (X(0,0) - A(0,0)))

-- smoothed length of the forward differences (a one-sided stencil)
for dx, dy in Stencil({ {1,0}, {0,1} }) do
    local d = X(0,0) - X(dx,dy)
    local len = Sqrt(d(0) * d(0) + d(1) * d(1) + eps * eps)
    Energy(Select(InBounds(dx,dy), w_regSqrt * (len - eps), 0))
end
