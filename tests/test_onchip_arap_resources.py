"""CPU test (no GPU): the one-workgroup ARAP linear solves (arap_onchipPcg<T, V, LMV>, opt_amd/csrc/arap_onchip.h; solver parameter amd_onchip = 5), read from the
compiler's resource remarks like tests/test_onchip_general_resources.py does: every offered variant exists, none uses scratch, each leaves room for its workgroup, and the
variants the GPU tests walk (tests/test_onchip_arap_gpu.py::ARAP_VARIANTS) are exactly the ones the library instantiates.

The register rule.  The kernel is launched as ONE workgroup of up to kAoMaxWaves = 8 waves (512 threads: 2 waves per SIMD), so a lane may use the 512 registers of its
SIMD lane divided by 2: VGPRs + AGPRs <= 256, and the remarks' occupancy (waves per SIMD the registers allow) must be at least 2 -- otherwise the 512-thread launch
would be refused.  (At 1024 threads and 128 registers every variant spilled, which is why the workgroup stops at 512.)
"""
import re

import pytest

from opt_amd import build
from test_onchip_arap_gpu import ARAP_VARIANTS

WAVES_PER_SIMD = 2      # 8 waves on 4 SIMDs


@pytest.fixture(scope="module")
def kernels(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    out = {}
    for name, r in build.kernel_resources().items():
        m = re.match(r"^arap_onchipPcg<(float|double), (\d+), (true|false)>$", name)
        if m:
            out[(m.group(1), int(m.group(2)), m.group(3) == "true")] = r
    return out


@pytest.mark.parametrize("prec,v,lmv", ARAP_VARIANTS)
def test_every_offered_variant_exists(kernels, prec, v, lmv):
    assert (prec, v, lmv) in kernels, sorted(kernels)


def test_no_such_kernel_uses_scratch(kernels):
    assert kernels and all(r["scratch"] == 0 for r in kernels.values()), {k: r["scratch"] for k, r in kernels.items() if r["scratch"]}


def test_each_leaves_room_for_its_workgroup(kernels):
    assert kernels
    for k, r in kernels.items():
        assert r["vgprs"] + r["agprs"] <= 512 // WAVES_PER_SIMD and r["occupancy"] >= WAVES_PER_SIMD, (k, r)


def test_static_lds_leaves_room_for_p_and_delta(kernels):
    """p and delta of up to V * 512 vertices are dynamic LDS (48 bytes per vertex in float, 96 in double): with the kernel's own static LDS (the sums' staging) the
    largest launch of every variant stays inside the 160 KB of a CU."""
    for (prec, v, lmv), r in kernels.items():
        assert r["lds"] + v * 512 * (48 if prec == "float" else 96) <= 160 * 1024, ((prec, v, lmv), r)


def test_the_gpu_tests_list_exactly_the_offered_variants(kernels):
    assert len(set(ARAP_VARIANTS)) == len(ARAP_VARIANTS)
    assert set(ARAP_VARIANTS) == set(kernels), (sorted(set(kernels) - set(ARAP_VARIANTS)), sorted(set(ARAP_VARIANTS) - set(kernels)))
