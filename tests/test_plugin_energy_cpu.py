"""CPU tests (no GPU needed) of energy plug-ins: include/OptAmdPlugin.h, OptAmd_LoadEnergyPlugin / OPT_AMD_ENERGY_PLUGINS, opt_amd/build.py build_plugin and the
shipped sample examples/plugins/spring_mesh_deformation.{t,hip} -- an energy that is not one of the built-in twelve.

The registry is process-global and tests/test_boundary.py enumerates it, so no plug-in is ever loaded in the pytest process: each test runs its body in a fresh
child (tests/plugin_energy_driver.py <case>), which prints one JSON line."""
import json
import os
import subprocess
import sys

import pytest

import plugin_energy_driver as drv
from opt_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "plugin_energy_driver.py")
BUILTINS = ["image_warping", "poisson_image_editing", "laplacian", "curveFitting", "arap_mesh_deformation", "shape_from_shading", "optical_flow",
            "intrinsic_image_decomposition", "volumetric_mesh_deformation", "cotangent_mesh_smoothing", "embedded_mesh_deformation", "robust_nonrigid_alignment"]
STEM = "spring_mesh_deformation"


def child(case, args=None, env=None, timeout=120):
    e = dict(os.environ)
    e.pop("OPT_AMD_ENERGY_PLUGINS", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, DRIVER, case, json.dumps(args or {})], capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


@pytest.fixture(scope="module")
def sample(opt_lib):
    """The sample plug-in, built once per session (hipcc cross-compiles it without a GPU)."""
    return build.build_plugin(build.SAMPLE_PLUGIN, force=False)


def test_build_helper_and_kernel_resources(opt_lib):
    """build_plugin cross-compiles the sample; its remarks list every engine kernel for the new functor in float and double, every one without scratch
    (the "no scratch in an offered variant" rule), and they stay out of opt_amd/build/ -- kernel_resources() of libOpt.so does not see the plug-in."""
    lib = build.build_plugin(build.SAMPLE_PLUGIN)
    assert lib == build.plugin_path(STEM) and os.path.exists(lib)
    assert os.path.dirname(lib) == os.path.join(os.path.dirname(opt_lib.LIB_PATH), "plugins")
    res = build.plugin_kernel_resources(STEM)
    for prec in ("float", "double"):
        G = "SpringG<%s>" % prec
        want = ["ge_vertices<%s, %s, %d, 1>" % (prec, G, m) for m in range(4)] + ["ge_vertices<%s, %s, %d, 4>" % (prec, G, m) for m in (2, 3)]
        want += ["ge_edges<%s, %s, %d>" % (prec, G, m) for m in range(4)]
        want += ["ge_gather<%s, %s, %s>" % (prec, G, c) for c in ("false", "true")] + ["ge_flatStep<%s, %s>" % (prec, c) for c in ("false", "true")]
        want += ["ge_onchipPcg<%s, %s, 1, %s>" % (prec, G, c) for c in ("false", "true")] + ["ge_onchipPcgGrid<%s, %s, %s>" % (prec, G, c) for c in ("false", "true")]
        for w in want:
            hits = [k for k in res if k.endswith(w)]
            assert len(hits) == 1, (w, sorted(res))
    spring = {k: v for k, v in res.items() if "SpringG" in k or "ge_flatStep" in k}
    assert len(spring) == 2 * 18
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
    assert not any("SpringG" in k for k in build.kernel_resources())
    assert not [f for f in os.listdir(build.OBJDIR) if STEM in f]
    # self-contained: nothing of libOpt.so is needed to load it (the linker was not given the library, and no symbol of its namespace is left undefined)
    und = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True).stdout
    assert "optamd" not in und and "OptAmd_" not in und and "Opt_" not in und, und


def test_refused_before_loading(opt_lib):
    """Without the plug-in the sample's .t has no kernel set (this is the test that fails without the feature: the driver's load cases need the loader)."""
    out, _ = child("before")
    assert not out["ok"] and "no hand-written kernel set" in out["message"], out
    assert out["names"] == BUILTINS
    assert hasattr(opt_lib, "load_energy_plugin") and "OptAmd_LoadEnergyPlugin" in opt_lib.OPTAMD_SYMBOLS


def test_after_loading_the_energy_is_like_a_built_in(sample, tmp_path):
    out, _ = child("load", {"plugin": sample, "tmp": str(tmp_path)})
    assert out["n"] == 1 and out["before"] == BUILTINS and out["names"] == BUILTINS + [STEM]      # count 13, the twelve unchanged and in order
    assert out["own"] == [True, "ok: " + STEM], out["own"]
    assert out["other_name"] == [True, "ok: " + STEM], out["other_name"]      # the same body under another file name resolves by its hash
    ok, msg = out["edited_body"]
    assert not ok and "energy body" in msg and out["hash"] in msg and "(plug-in)" in msg, msg      # ... an edited Energy line is refused, the accepted hash listed
    assert out["hash"] in open(build.SAMPLE_PLUGIN).read()
    ok, msg = out["moved_index"]
    assert not ok and "UrShape" in msg and "index 4" in msg, msg      # validate() applies unchanged
    assert out["builtin"] == [True, "ok: embedded_mesh_deformation"]


def test_refusals_leave_the_registry_alone(sample, opt_lib, tmp_path):
    skew = build.build_plugin(build.SAMPLE_PLUGIN, out=str(tmp_path / "libspring_abi_skew.so"), defines=["OPTAMD_PLUGIN_ABI_SKEW=1"])
    dup = build.build_plugin(os.path.join(HERE, "plugin_sources", "duplicate_name.hip"), out=str(tmp_path / "libduplicate_name.so"))
    comm = os.path.join(os.path.dirname(opt_lib.LIB_PATH), "libOptComm.so")
    assert os.path.exists(comm)
    out, _ = child("refusals", {"missing": str(tmp_path / "nope.so"), "no_entry": comm, "abi_skew": skew, "duplicate_builtin": dup, "sample": sample, "sample_again": sample})
    assert out["count0"] == 12
    words = {"missing": "cannot open", "no_entry": "does not export", "abi_skew": "ABI stamp", "duplicate_builtin": "'image_warping'"}
    for key, word in words.items():
        r = out[key]
        assert r["n"] == -1 and word in r["message"] and r["count"] == 12, (key, r)
    assert out["sample"] == {"n": 1, "message": "", "count": 13}
    r = out["sample_again"]
    assert r["n"] == -1 and "already registered" in r["message"] and STEM in r["message"] and r["count"] == 13, r
    assert len({out[k]["message"] for k in list(words) + ["sample_again"]}) == 5      # every refusal says something else
    assert out["names"] == BUILTINS + [STEM]


def test_environment_route(sample):
    """OPT_AMD_ENERGY_PLUGINS is read by the first Opt_NewState: nothing before it; on a machine without a GPU the state is still NULL, and the registry holds
    the plug-in afterwards.  A path that is refused is reported on stderr and the rest of the list is still loaded."""
    import torch
    out, err = child("env", env={"OPT_AMD_ENERGY_PLUGINS": "/nonexistent/libnope.so:" + sample})
    assert out["before"] == BUILTINS
    assert out["state"] == torch.cuda.is_available()
    assert out["names"] == BUILTINS + [STEM] and out["check"] == [True, "ok: " + STEM], (out, err)
    assert "OPT_AMD_ENERGY_PLUGINS" in err and "cannot open" in err and "libnope.so" in err, err
    out, err = child("env")
    assert out["names"] == BUILTINS and "OPT_AMD_ENERGY_PLUGINS" not in err


def test_the_builders_give_the_meshes_the_gpu_tests_name():
    for mesh, n in (("grid", 35), ("armadillo", 130), ("grid_shapes", 36)):
        for double in (False, True):
            P = drv.problem(mesh, double)
            assert P.dims == (n,) and P.params[0].shape == (n, 3) and P.params[0].dtype == (float if double else "float32")
            h, t = P.params[6], P.params[7]
            assert len(h) == len(t) == int(P.params[5]) and h.min() >= 0 and max(h.max(), t.max()) < n
            import numpy as np
            d = np.linalg.norm(P.params[0][t].astype(float) - P.params[0][h].astype(float), axis=1)
            assert d.min() > 1e-3      # no two joined vertices coincide: the edge length is differentiable everywhere the tests go
    P = drv.problem("grid_shapes", True)
    import numpy as np
    deg = np.bincount(P.params[6], minlength=36)
    assert deg[35] == 0 and deg[17] == 16 and not np.any(P.params[7] == 35)
