"""CPU test (no GPU): the on-chip image_warping kernels for a general UrShape (iw_onchipPcgGeneral<T, ROWS, LMV>, opt_amd/csrc/iw_onchip.h; solver parameter amd_onchip = 4), read
from the compiler's resource remarks like tests/test_kernel_resources.py does: every required variant exists, none uses scratch, each leaves room for its 8-wave workgroup, the
variants the GPU tests force one by one (tests/test_onchip_general_gpu.py::GENERAL_VARIANTS) are exactly the ones the library instantiates -- and the unit-lattice kernels
iw_onchipPcg<...>, whose body the general kernels share, still compile to the registers and scratch they had before the body was shared.
"""
import re

import pytest

from opt_amd import build
from test_onchip_general_gpu import GENERAL_VARIANTS

REQUIRED = [("float", 2, False), ("float", 4, False), ("float", 2, True), ("float", 4, True), ("double", 2, False), ("double", 2, True)]

# iw_onchipPcg<T, ROWS, AP_LDS, DELTA_GLB, LMV>: (VGPRs, scratch bytes per lane)
LATTICE_KERNELS = {
    "iw_onchipPcg<float, 2, false, false, false>": (105, 0), "iw_onchipPcg<float, 2, false, false, true>": (117, 0),
    "iw_onchipPcg<float, 4, false, false, false>": (146, 0), "iw_onchipPcg<float, 4, false, false, true>": (173, 0),
    "iw_onchipPcg<float, 8, false, false, false>": (246, 0), "iw_onchipPcg<float, 8, false, false, true>": (256, 76),
    "iw_onchipPcg<float, 16, true, true, false>": (256, 40),
    "iw_onchipPcg<double, 2, false, false, false>": (168, 0), "iw_onchipPcg<double, 2, false, false, true>": (197, 0),
    "iw_onchipPcg<double, 4, false, false, false>": (256, 0),
}


@pytest.fixture(scope="module")
def resources(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    return build.kernel_resources()


@pytest.fixture(scope="module")
def general(resources):
    out = {}
    for name, r in resources.items():
        m = re.match(r"^iw_onchipPcgGeneral<(float|double), (\d+), (true|false)>$", name)
        if m:
            out[(m.group(1), int(m.group(2)), m.group(3) == "true")] = r
    return out


@pytest.mark.parametrize("prec,rows,lmv", REQUIRED)
def test_every_required_variant_exists(general, prec, rows, lmv):
    assert (prec, rows, lmv) in general, sorted(general)


def test_no_such_kernel_uses_scratch(general):
    assert general and all(r["scratch"] == 0 for r in general.values()), {k: r["scratch"] for k, r in general.items() if r["scratch"]}


def test_each_leaves_room_for_its_workgroup(general):
    """8 waves = 2 per SIMD: at most 256 registers per lane, and the register budget must allow 2 waves per SIMD."""
    assert general
    for k, r in general.items():
        assert r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] >= 2, (k, r)


def test_the_gpu_tests_list_exactly_the_offered_variants(general):
    assert len(set(GENERAL_VARIANTS)) == len(GENERAL_VARIANTS)
    assert set(GENERAL_VARIANTS) == set(general), (sorted(set(general) - set(GENERAL_VARIANTS)), sorted(set(GENERAL_VARIANTS) - set(general)))


def test_the_unit_lattice_kernels_kept_their_registers(resources):
    have = {n: (r["vgprs"], r["scratch"]) for n, r in resources.items() if n.startswith("iw_onchipPcg<")}
    assert have == LATTICE_KERNELS, {n: (have.get(n), LATTICE_KERNELS.get(n)) for n in set(have) | set(LATTICE_KERNELS) if have.get(n) != LATTICE_KERNELS.get(n)}
