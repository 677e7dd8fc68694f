"""CPU test (no GPU): the on-chip Levenberg-Marquardt kernels with the split residual reset inside the solve (march_onchipPcg<T, Op, rows, waves, 2>,
opt_amd/csrc/stencil_onchip.h), read from the compiler's resource remarks like tests/test_kernel_resources.py does: every (operator, precision) pair of the 5-point-stencil
family offers at least one, none of them uses scratch, and the variants the GPU tests force one by one (tests/test_onchip_reset_gpu.py::MODE2_VARIANTS) are exactly the ones
the library instantiates -- no offered variant goes untested, no listed one is missing.
"""
import re

import pytest

from opt_amd import build
from test_onchip_reset_gpu import MODE2_VARIANTS

OPERATORS = {"PoissonMarchOp": "poisson", "LaplacianMarchOp": "laplacian", "FlowMarchOp": "optical_flow", "IntrinsicMarchOp": "intrinsic"}
PAIRS = [("poisson", "float"), ("poisson", "double"), ("laplacian", "float"), ("optical_flow", "float"), ("optical_flow", "double"), ("intrinsic", "float"), ("intrinsic", "double")]


@pytest.fixture(scope="module")
def mode2(opt_lib):
    build.build()      # (re)compiles whatever has no remarks file yet
    out = {}
    for name, r in build.kernel_resources().items():
        m = re.match(r"^march_onchipPcg<(float|double), (\w+?)(?:<\w+>)?, (\d+), (\d+), 2>$", name)
        if m:
            out[(OPERATORS[m.group(2)], m.group(1), int(m.group(3)), int(m.group(4)))] = r
    return out


@pytest.mark.parametrize("op,prec", PAIRS)
def test_every_operator_and_precision_offers_the_reset_on_chip(mode2, op, prec):
    assert [k for k in mode2 if k[:2] == (op, prec)], sorted(mode2)


def test_no_such_kernel_uses_scratch(mode2):
    assert mode2 and all(r["scratch"] == 0 for r in mode2.values()), {k: r["scratch"] for k, r in mode2.items() if r["scratch"]}


def test_the_gpu_tests_list_exactly_the_offered_variants(mode2):
    assert len(set(MODE2_VARIANTS)) == len(MODE2_VARIANTS)
    assert set(MODE2_VARIANTS) == set(mode2), (sorted(set(mode2) - set(MODE2_VARIANTS)), sorted(set(MODE2_VARIANTS) - set(mode2)))
