"""CPU test (no GPU): the one-workgroup linear solves of the functor mesh energies (ge_onchipPcg<T, G, V, LMV>, opt_amd/csrc/graph_onchip.h; solver parameter
amd_onchip = 6), read from the compiler's resource remarks like tests/test_onchip_arap_resources.py does: every variant the GPU tests list
(tests/test_onchip_graph_gpu.py::GRAPH_VARIANTS) exists, the list is exactly the instantiated set, none uses scratch, each leaves room for its workgroup of 512 threads,
and its static plus dynamic LDS at the variant's largest mesh stays inside the 160 KB of a CU.

The kernels the path stands beside keep the registers, scratch and LDS they have on the parent commit: ge_edges / ge_vertices (tests/golden/graph_engine_resources.json),
ge_gather, ge_flatStep and arap_onchipPcg, whose workgroup sum moved to onchip_sync.h (tests/golden/graph_onchip_resources.json, written from the parent commit's build).
"""
import json
import os
import re

import pytest

from opt_amd import build
from test_onchip_graph_gpu import GRAPH_VARIANTS, LANES

HERE = os.path.dirname(os.path.abspath(__file__))
WAVES_PER_SIMD = 2      # 8 waves on 4 SIMDs
K = {"CotangentG": 3, "EmbeddedG": 12, "RobustG": 7}      # unknowns per vertex
# solver vectors of K scalars per vertex in LDS: p and delta; in double embedded keeps r there too and cotangent r and A p (G::kOnChipLdsVectors)
LDS_VECTORS = {("float", "CotangentG"): 2, ("float", "EmbeddedG"): 2, ("float", "RobustG"): 2, ("double", "CotangentG"): 4, ("double", "EmbeddedG"): 3, ("double", "RobustG"): 2}


@pytest.fixture(scope="module")
def resources(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    return build.kernel_resources()


@pytest.fixture(scope="module")
def kernels(resources):
    out = {}
    for name, r in resources.items():
        m = re.match(r"^ge_onchipPcg<(float|double), (?:optamd::)?(?:\(anonymous namespace\)::)?(\w+)<(float|double)>, (\d+), (true|false)>$", name)
        if m:
            assert m.group(1) == m.group(3), name
            out[(m.group(1), m.group(2), int(m.group(4)), m.group(5) == "true")] = r
    return out


@pytest.mark.parametrize("prec,functor,v,lm", GRAPH_VARIANTS)
def test_every_listed_variant_exists(kernels, prec, functor, v, lm):
    assert (prec, functor, v, lm) in kernels, sorted(kernels)


def test_the_gpu_tests_list_exactly_the_instantiated_variants(kernels):
    assert len(set(GRAPH_VARIANTS)) == len(GRAPH_VARIANTS)
    assert set(GRAPH_VARIANTS) == set(kernels), (sorted(set(kernels) - set(GRAPH_VARIANTS)), sorted(set(GRAPH_VARIANTS) - set(kernels)))


@pytest.mark.parametrize("functor", sorted(K))
@pytest.mark.parametrize("lm", [False, True])
def test_the_required_variants_are_offered(kernels, functor, lm):
    assert ("float", functor, 1, lm) in kernels
    assert ("float", "CotangentG", 2, lm) in kernels      # head.ply: 689 vertices


def test_no_offered_variant_uses_scratch(kernels):
    assert kernels and all(r["scratch"] == 0 for r in kernels.values()), {k: r["scratch"] for k, r in kernels.items() if r["scratch"]}


def test_each_leaves_room_for_its_workgroup(kernels):
    assert kernels
    for k, r in kernels.items():
        assert r["vgprs"] + r["agprs"] <= 512 // WAVES_PER_SIMD and r["occupancy"] >= WAVES_PER_SIMD, (k, r)


def test_lds_at_the_largest_mesh_fits_the_cu(kernels):
    for (prec, functor, v, lm), r in kernels.items():
        dynamic = v * LANES * LDS_VECTORS[(prec, functor)] * K[functor] * (4 if prec == "float" else 8)
        assert r["lds"] + dynamic <= 160 * 1024, ((prec, functor, v, lm), r, dynamic)


@pytest.mark.parametrize("golden,count", [("graph_engine_resources.json", 60), ("graph_onchip_resources.json", 23)])
def test_the_kernels_beside_the_path_keep_their_resources(resources, golden, count):
    """arap_onchipPcg, ge_edges, ge_vertices, ge_gather and ge_flatStep: VGPRs, AGPRs, SGPRs, scratch and LDS of the parent commit's build."""
    want = json.load(open(os.path.join(HERE, "golden", golden)))
    assert len(want) == count
    for name, w in want.items():
        assert name in resources, name
        got = {k: resources[name][k] for k in w}
        assert got == w, (name, got, w)
    if golden == "graph_onchip_resources.json":
        assert sum("arap_onchipPcg" in n for n in want) == 7 and sum("ge_gather" in n for n in want) == 12 and sum("ge_flatStep" in n for n in want) == 4
