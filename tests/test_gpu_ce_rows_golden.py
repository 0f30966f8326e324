"""GPU: the row cross-entropy entry points of csrc/loss.hip (capmi_ce_fwd_bwd, capmi_ce_ignore_fwd_bwd,
capmi_pg_ce_fwd_bwd, capmi_count_targets, capmi_loss_finalize, capmi_loss_finalize_dev) give, bit for bit, what the
three separate kernels gave before they were merged into one definition.

tests/golden/ce_rows.npz is device-recorded: it holds the outputs, as 32-bit integer patterns, that the library
built from the commit before the merge wrote on an MI355X for the cases of tests/ce_rows_cases.py (cases, inputs
and what is stored: that file's docstring). Nothing in it comes from a CPU reference, so it pins the operation
order, not the accuracy (tests/test_gpu_decoder_kernels.py, tests/test_gpu_baseline_train_kernels.py and
tests/test_gpu_scst.py hold these kernels to fp64). To regenerate it, on an MI355X, with the build to pin:

    CAPMI_LIB=<that build's libcapmi.so> python tools/make_ce_rows_golden.py

and only together with a deliberate change of the row arithmetic."""
import numpy as np
import pytest

import ce_rows_cases as C

pytestmark = pytest.mark.gpu
CASES = C.cases()


@pytest.fixture(scope="module")
def pinned():
    z = np.load(C.GOLDEN)
    return {k: z[k] for k in z.files}


def test_fixture_holds_exactly_the_case_list(pinned):
    assert {k.split("/")[0] for k in pinned} == {c[0] for c in CASES}
    assert all(a.any() for a in pinned.values()), "an all-zero array pins nothing"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bit_equal_to_the_recorded_rows(case, pinned):
    from capmi import kernels as K
    got = C.run(case, K)
    want = {k.split("/")[1]: a for k, a in pinned.items() if k.split("/")[0] == case[0]}
    assert set(got) == set(want), f"{case[0]}: outputs {sorted(got)}, recorded {sorted(want)}"
    for name, a in got.items():
        w = want[name]
        assert a.dtype == w.dtype and a.shape == w.shape, f"{case[0]} {name}: {a.dtype}{a.shape} vs {w.dtype}{w.shape}"
        bad = np.argwhere(a != w)
        assert len(bad) == 0, (f"{case[0]} {name}: {len(bad)} of {a.size} patterns differ, first at {bad[0].tolist()}: "
                               f"{int(a[tuple(bad[0])]):#010x}, recorded {int(w[tuple(bad[0])]):#010x}")
