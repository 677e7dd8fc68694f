"""CPU tests (no GPU needed) of image-domain energy plug-ins: stencilEnergyInfo of include/OptAmdPlugin.h, the shipped sample
examples/plugins/vector_tv_denoising.{t,hip} -- an energy that is not one of the built-in twelve -- and the kernels of the two-launch PCG iteration of the functor
stencil engine (solver parameter amd_stencil_fused = 1; opt_amd/csrc/stencil_engine.h se_gatherIter, graph_pcg.h ge_flatStep / ge_flatStepNoPre), read from the
compiler's resource remarks as tests/test_kernel_resources.py reads them.

No plug-in is loaded in the pytest process (the registry is process-global): the loader runs in a fresh child (tests/stencil_plugin_driver.py).  A plan cannot be
made without a device (Opt_NewState returns NULL), so what OptAmd_PlanDescribe says under amd_stencil_fused = 1 is checked by tests/test_stencil_plugin_gpu.py."""
import json
import os
import re
import subprocess
import sys

import pytest

from opt_amd import build, workloads as wl

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "stencil_plugin_driver.py")
STEM = "vector_tv_denoising"
BUILTINS = ["image_warping", "poisson_image_editing", "laplacian", "curveFitting", "arap_mesh_deformation", "shape_from_shading", "optical_flow",
            "intrinsic_image_decomposition", "volumetric_mesh_deformation", "cotangent_mesh_smoothing", "embedded_mesh_deformation", "robust_nonrigid_alignment"]
ITER_VARIANTS = [(lm, pre) for lm in ("false", "true") for pre in ("false", "true")]      # se_gatherIter<T, E, LM, PRE>


def test_build_helper_and_kernel_resources(opt_lib):
    """build_plugin cross-compiles the sample for gfx950; its remarks list every engine kernel for the new functor in float and double, every one of them --
    the se_gatherIter instantiations included -- without scratch; they stay out of opt_amd/build/; the library is self-contained."""
    lib = build.build_plugin(build.SAMPLE_STENCIL_PLUGIN)
    assert lib == build.plugin_path(STEM) and os.path.exists(lib)
    res = build.plugin_kernel_resources(STEM)
    for prec in ("float", "double"):
        E = "VectorTvE<%s>" % prec
        want = ["se_cost<%s, %s >" % (prec, E), "se_modelCost<%s, %s >" % (prec, E)] + ["se_gather<%s, %s, %s>" % (prec, E, c) for c in ("false", "true")]
        want += ["se_gatherIter<%s, %s, %s, %s>" % (prec, E, lm, pre) for lm, pre in ITER_VARIANTS]
        want += ["ge_flatStep<%s, %s>" % (prec, c) for c in ("false", "true")] + ["ge_flatStepNoPre<%s, %s>" % (prec, c) for c in ("false", "true")]
        for w in want:
            hits = [k for k in res if k.endswith(w)]
            assert len(hits) == 1, (w, sorted(res))
    assert len(res) == 2 * 12, sorted(res)      # nothing of the marching template or the on-chip stencil solves: plug-in sources do not get them
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
    assert not any("VectorTvE" in k for k in build.kernel_resources())
    assert not [f for f in os.listdir(build.OBJDIR) if STEM in f]
    und = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True).stdout
    assert "optamd" not in und and "OptAmd_" not in und and "Opt_" not in und, und


@pytest.fixture(scope="module")
def resources(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    return build.kernel_resources()


@pytest.mark.parametrize("functor", ["OpticalFlowE", "IntrinsicE", "VolumetricE"])
@pytest.mark.parametrize("prec", ["float", "double"])
def test_the_gather_of_every_built_in_functor_needs_no_scratch(resources, functor, prec):
    """se_gatherIter<T, E, LM, PRE> in the library's own remarks: all four (LM, PRE) variants of the three built-in functors exist, in float and double, without scratch
    (the walk of IntrinsicE and VolumetricE in double is register-heavy: an instantiation that spilled at kBlock threads would need a smaller launch bound)."""
    for lm, pre in ITER_VARIANTS:
        name = "optamd::se_gatherIter<%s, %s<%s>, %s, %s>" % (prec, functor, prec, lm, pre)
        assert name in resources, (name, sorted(k for k in resources if "se_gatherIter" in k))
        r = resources[name]
        assert r["scratch"] == 0 and r["lds"] == 160, (name, r)      # LDS: the four sums' staging, 4 * (256 / 64 + 1) doubles
        # it holds what se_gather<T, E, true> holds plus the sums: never fewer registers' worth of occupancy than a kernel that ran before
        assert r["occupancy"] >= 1


@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("lm", ["false", "true"])
def test_the_flat_passes_exist_without_scratch(resources, prec, lm):
    for k in ("optamd::ge_flatStep<%s, %s>" % (prec, lm), "optamd::ge_flatStepNoPre<%s, %s>" % (prec, lm)):
        r = resources[k]
        assert r["scratch"] == 0 and r["occupancy"] == 8 and r["lds"] == 160, (k, r)
    # the flat pass lives in one place: both engines' translation units instantiate the same text
    src = {f: open(os.path.join(build.CSRC, f)).read() for f in ("graph_pcg.h", "graph_engine.h", "stencil_engine.h")}
    assert len(re.findall(r"void ge_flatStep\(", src["graph_pcg.h"])) == 1 and "void ge_flatStep(" not in src["graph_engine.h"] + src["stencil_engine.h"]


def child(case, args=None, timeout=120):
    e = dict(os.environ)
    e.pop("OPT_AMD_ENERGY_PLUGINS", None)
    r = subprocess.run([sys.executable, DRIVER, case, json.dumps(args or {})], capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_loader_accepts_the_sample_and_its_t_matches_params(opt_lib, tmp_path):
    """In a child: refused before loading, accepted after; the .t's declarations match `params` (kind, name, type, binding index, UsePreconditioner) -- the same
    validation as for a built-in energy, shown by the three edits it refuses -- and the recorded hash is the file's."""
    sample = build.build_plugin(build.SAMPLE_STENCIL_PLUGIN, force=False)
    out = child("load", {"plugin": sample, "tmp": str(tmp_path)})
    ok, msg = out["refused_before"]
    assert not ok and "no hand-written kernel set" in msg, msg
    assert out["n"] == 1 and out["before"] == BUILTINS and out["names"] == BUILTINS + [STEM]
    assert out["own"] == [True, "ok: " + STEM], out["own"]
    assert out["hash"] in open(build.SAMPLE_STENCIL_PLUGIN).read()
    ok, msg = out["moved_index"]
    assert not ok and '"A"' in msg and "index 4" in msg, msg
    ok, msg = out["retyped"]
    assert not ok and "Mask" in msg and "opt_float2" in msg, msg
    ok, msg = out["no_preconditioner"]
    assert not ok and "UsePreconditioner" in msg, msg


def test_the_declarations_of_the_t_are_the_builder_s_slots():
    """The synthetic-input builder fills the slots the .t declares: X, A (two channels), Mask (one), three host floats."""
    import numpy as np
    src = open(wl.VECTOR_TV_T).read()
    decl = re.findall(r'(Unknown|Array|Param)\("(\w+)",\s*(\w+),\s*(?:\{W,H\},\s*)?(\d+)\)', src)
    assert decl == [("Unknown", "X", "opt_float2", "0"), ("Array", "A", "opt_float2", "1"), ("Array", "Mask", "opt_float", "2"),
                    ("Param", "w_fitSqrt", "float", "3"), ("Param", "w_regSqrt", "float", "4"), ("Param", "eps", "float", "5")], decl
    assert "UsePreconditioner(true)" in src and "Exclude(greater(Mask(0,0), 0))" in src
    for double in (False, True):
        P = wl.vector_tv_denoising(13, 9, double=double, seed=1, mask="block")
        ft = np.float64 if double else np.float32
        assert P.energy == STEM and P.dims == (13, 9) and len(P.params) == 6
        assert P.params[0].shape == (9, 13, 2) and P.params[1].shape == (9, 13, 2) and P.params[2].shape == (9, 13)
        assert all(P.params[i].dtype == ft for i in range(3)) and all(np.asarray(P.params[i]).dtype == np.float32 and np.ndim(P.params[i]) == 0 for i in (3, 4, 5))
        assert float(P.params[5]) > 0
