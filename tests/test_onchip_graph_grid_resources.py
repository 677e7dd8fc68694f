"""CPU test (no GPU): the several-workgroup linear solves of the functor mesh energies (ge_onchipPcgGrid<T, G, LMV>, opt_amd/csrc/graph_onchip_grid.h; solver
parameter amd_onchip = 7), read from the compiler's resource remarks like tests/test_onchip_graph_resources.py does: all twelve kernels exist (three functors x float /
double x Gauss-Newton / Levenberg-Marquardt), none uses scratch, each leaves room for its workgroup of 512 threads, and its static LDS plus the largest dynamic LDS the
host grants (GraphOps::kGgLdsBudget) stays inside the 160 KB of a CU.

ge_onchipPcg shares its edge and vertex phases with the new kernel (geOcEdges, geOcVertex gained a view of one part of a partition): its sixteen kernels keep the VGPRs,
AGPRs, SGPRs, scratch and LDS of the parent commit's build (tests/golden/graph_onchip_grid_parent_resources.json, written from the parent commit's build).
"""
import json
import os
import re

import pytest

from opt_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
WAVES_PER_SIMD = 2      # 8 waves on 4 SIMDs
FUNCTORS = ("CotangentG", "EmbeddedG", "RobustG")
GRID_KERNELS = [(p, f, lm) for p in ("float", "double") for f in FUNCTORS for lm in (False, True)]      # none is withheld
DYNAMIC_LDS_BUDGET = 160 * 1024 - 4096      # graph_engine.h GraphOps::kGgLdsBudget


@pytest.fixture(scope="module")
def resources(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    return build.kernel_resources()


@pytest.fixture(scope="module")
def kernels(resources):
    out = {}
    for name, r in resources.items():
        m = re.match(r"^ge_onchipPcgGrid<(float|double), (?:optamd::)?(?:\(anonymous namespace\)::)?(\w+)<(float|double)>, (true|false)>$", name)
        if m:
            assert m.group(1) == m.group(3), name
            out[(m.group(1), m.group(2), m.group(4) == "true")] = r
    return out


@pytest.mark.parametrize("prec,functor,lm", GRID_KERNELS)
def test_every_kernel_exists(kernels, prec, functor, lm):
    assert (prec, functor, lm) in kernels, sorted(kernels)


def test_the_list_is_exactly_the_instantiated_set(kernels):
    assert len(GRID_KERNELS) == 12 and set(GRID_KERNELS) == set(kernels), (sorted(set(kernels) - set(GRID_KERNELS)), sorted(set(GRID_KERNELS) - set(kernels)))


def test_the_name_stays_clear_of_the_one_workgroup_kernels(resources):
    assert not any(re.match(r"^ge_onchipPcg<", n) and "Grid" in n for n in resources)
    assert sum(1 for n in resources if re.match(r"^ge_onchipPcg<", n)) == 16


def test_no_kernel_uses_scratch(kernels):
    assert kernels and all(r["scratch"] == 0 for r in kernels.values()), {k: r["scratch"] for k, r in kernels.items() if r["scratch"]}


def test_each_leaves_room_for_its_workgroup(kernels):
    assert kernels
    for k, r in kernels.items():
        assert r["vgprs"] + r["agprs"] <= 512 // WAVES_PER_SIMD and r["occupancy"] >= WAVES_PER_SIMD, (k, r)


def test_static_plus_the_largest_dynamic_lds_fits_the_cu(kernels):
    assert kernels
    for k, r in kernels.items():
        assert r["lds"] + DYNAMIC_LDS_BUDGET <= 160 * 1024, (k, r)


def test_the_one_workgroup_kernels_keep_their_resources(resources):
    want = json.load(open(os.path.join(HERE, "golden", "graph_onchip_grid_parent_resources.json")))
    assert len(want) == 16 and all(n.startswith("ge_onchipPcg<") for n in want)
    for name, w in want.items():
        assert name in resources, name
        got = {k: resources[name][k] for k in w}
        assert got == w, (name, got, w)
