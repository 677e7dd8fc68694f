"""CPU test (no GPU): the kernels of the two-launch PCG iteration of the functor mesh energies (ge_gather<T, G, LM>, ge_flatStep<T, LM>; opt_amd/csrc/graph_engine.h,
solver parameter amd_graph_fused = 1), read from the compiler's resource remarks like tests/test_onchip_arap_resources.py does.

The rule: a gather instantiation may not use more scratch than ge_edges<T, G, 3> of the same energy and precision -- the kernel it replaces, from the same remarks --
and the float instantiations of all three energies must be offered.  ge_edges / ge_vertices themselves keep the registers, scratch and LDS they had before the
path existed (tests/golden/graph_engine_resources.json, written from the parent commit's build)."""
import json
import os
import re

import pytest

from opt_amd import build
from test_graph_fused_gpu import GATHER_VARIANTS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_engine_resources.json")


@pytest.fixture(scope="module")
def resources(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    return build.kernel_resources()


@pytest.fixture(scope="module")
def gathers(resources):
    out = {}
    for name, r in resources.items():
        m = re.match(r"^optamd::ge_gather<(float|double), (\w+)<(float|double)>, (true|false)>$", name)
        if m:
            assert m.group(1) == m.group(3), name
            out[(m.group(1), m.group(2), m.group(4) == "true")] = r
    return out


@pytest.mark.parametrize("prec,functor,lm", GATHER_VARIANTS)
def test_every_listed_gather_exists(gathers, prec, functor, lm):
    assert (prec, functor, lm) in gathers, sorted(gathers)


def test_the_gpu_tests_list_exactly_the_instantiated_gathers(gathers):
    assert len(set(GATHER_VARIANTS)) == len(GATHER_VARIANTS)
    assert set(GATHER_VARIANTS) == set(gathers), (sorted(set(gathers) - set(GATHER_VARIANTS)), sorted(set(GATHER_VARIANTS) - set(gathers)))


def test_no_gather_uses_more_scratch_than_the_edge_pass_it_replaces(resources, gathers):
    assert gathers
    for (prec, functor, lm), r in gathers.items():
        edges = resources[f"optamd::ge_edges<{prec}, {functor}<{prec}>, 3>"]
        assert r["scratch"] <= edges["scratch"], ((prec, functor, lm), r, edges)


@pytest.mark.parametrize("functor", ["CotangentG", "EmbeddedG", "RobustG"])
@pytest.mark.parametrize("lm", [False, True])
def test_the_float_gathers_are_offered(gathers, functor, lm):
    assert ("float", functor, lm) in gathers


@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("lm", ["false", "true"])
def test_the_flat_step_exists_without_scratch(resources, prec, lm):
    r = resources[f"optamd::ge_flatStep<{prec}, {lm}>"]
    assert r["scratch"] == 0 and r["occupancy"] == 8, r


def test_the_record_kernels_keep_their_resources(resources):
    want = json.load(open(GOLDEN))
    assert len(want) == 60
    for name, w in want.items():
        assert name in resources, name
        got = {k: resources[name][k] for k in w}
        assert got == w, (name, got, w)
