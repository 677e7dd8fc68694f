"""CPU test (no GPU): shape_from_shading's on-chip Levenberg-Marquardt kernels with the split residual reset inside the solve (sfs_onchipPcg<T, rows, 2, waves>,
opt_amd/csrc/sfs_onchip.h), read from the compiler's resource remarks like tests/test_kernel_resources.py does: none of them uses scratch, float and double each offer one
that serves the reference's own 640 x 480 input, and the variants the GPU tests force one by one (tests/test_onchip_sfs_reset_gpu.py::SFS_MODE2_VARIANTS) are exactly the
ones the library instantiates -- no offered variant goes untested, no listed one is missing.
"""
import re

import pytest

from opt_amd import build
from test_onchip_sfs_reset_gpu import SFS_MODE2_VARIANTS

SPAN, MAX_WORKGROUPS = 60, 256      # pixels a wave owns per row (kSoSpan); one workgroup per CU (kSoMaxG)


@pytest.fixture(scope="module")
def mode2(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    out = {}
    for name, r in build.kernel_resources().items():
        m = re.match(r"^sfs_onchipPcg<(float|double), (\d+), 2, (\d+)>$", name)
        if m:
            out[(m.group(1), int(m.group(2)), int(m.group(3)))] = r
    return out


def test_no_such_kernel_uses_scratch(mode2):
    assert mode2 and all(r["scratch"] == 0 for r in mode2.values()), {k: r["scratch"] for k, r in mode2.items() if r["scratch"]}


@pytest.mark.parametrize("prec", ["float", "double"])
def test_a_variant_serves_the_reference_input(mode2, prec):
    """640 x 480 (examples/shape_from_shading/src/main.cpp:27-38): ceil(640 / 60) strips x ceil(480 / rows) tiles, `waves` of them per workgroup, one workgroup per CU"""
    fits = [(p, r, w) for (p, r, w) in mode2 if p == prec and -(-(-(-640 // SPAN) * -(-480 // r)) // w) <= MAX_WORKGROUPS]
    assert fits, sorted(mode2)


def test_the_gpu_tests_list_exactly_the_offered_variants(mode2):
    assert len(set(SFS_MODE2_VARIANTS)) == len(SFS_MODE2_VARIANTS)
    assert set(SFS_MODE2_VARIANTS) == set(mode2), (sorted(set(mode2) - set(SFS_MODE2_VARIANTS)), sorted(set(SFS_MODE2_VARIANTS) - set(mode2)))
