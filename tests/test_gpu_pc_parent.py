"""The sampler's element-wise tail against the bits recorded before its plain and guided kernels became one set
(tests/golden/pc_update_parent.npz, written by tests/golden/make_golden_pc_parent.py from tests/pc_parent_cases.py): the norm sums of
both traversals, plain and guided predictor-corrector steps under the VE and VP SDEs, a whole VP run and the fused DDIM route."""
import numpy as np
import pytest

import pc_parent_cases as P
from helpers import load_golden

pytestmark = pytest.mark.gpu


def _same_bits(got, want):
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("part", [P.norm_sums, P.pc_runs, P.ddim_runs])
def test_tail_reproduces_the_recorded_parent_bit_for_bit(part):
    want = load_golden("pc_update_parent")
    got = {}
    part(got)
    assert got and set(got) <= set(want)
    bad = [k for k in got if not _same_bits(got[k], want[k])]
    assert not bad, bad


def test_every_recorded_entry_is_compared():
    """The three parts above cover the fixture: its keys are exactly what they return (names only, no GPU work repeated)."""
    import itertools
    want = set(load_golden("pc_update_parent")) - {"commit"}
    names = {f"pc_{n}_{k}" for n in P.PC_RUNS for k in ("x", "x_mean")} | {"vp_run", "ddim_guided", "ddim_w1"}
    for B, n in itertools.product(P.NORM_B, P.NORM_PER_SAMPLE):
        names.add(f"norms_plain_B{B}_n{n}")
        names |= {f"norms_guided_B{B}_n{n}_ou{g}_scale{s}" for g in (0, 1) for s in P.NORM_SCALES}
    assert want == names
