"""CPU: what the attention captioner's self-critical step adds that can be checked without a GPU. The grouped
attention-backward entry points (csrc/att_group.hip) are declared, bound and validate their arguments before any
launch; the fp64 grouped references of tests/att_group_cases.py (the decoder_kernel_cases references on replicated
features, what tests/test_gpu_att_group.py holds the kernels to) equal a direct restatement that replicates
nothing; the step's constructor refuses what it does not take; train.py still does not dispatch to it."""
import ctypes
import re
import os

import pytest
import torch

import att_group_cases as GC
import decoder_kernel_cases as DC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capmi_att_group_bwd", "capmi_att_group_enc_grad")


def test_entry_points_are_declared_and_bound_without_an_abi_bump():
    import capmi
    from capmi import kernels as K
    with open(os.path.join(REPO, "include", "capmi.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capmi.EXPORTS and hasattr(capmi.lib, name)
    assert capmi.ABI_VERSION == 27 == capmi.lib.capmi_abi_version()
    assert callable(K.att_group_bwd) and callable(K.att_group_enc_grad)
    z = torch.zeros(4)
    with pytest.raises(ValueError):  # host tensors are refused: there is no CPU fallback
        K.att_group_bwd(z, 1, 0, z, z, z, z, 1, z, z, z, 1, 1, 1, 4, 4, z, z, z, z)
    with pytest.raises(ValueError):
        K.att_group_enc_grad(z, z, z, z, 1, 1, 1, 1, 4, z, z, z)


def _buf():
    raw = (ctypes.c_float * 80)()
    q = ctypes.addressof(raw)
    return raw, (q + 15) & ~15


def test_att_group_bwd_rejects_bad_arguments_before_any_launch():
    """CAPMI_EINVAL (1001) / CAPMI_ERANGE (1003): runs without a GPU."""
    import capmi
    raw, q = _buf()
    # dx_part S slab gate awe enc alpha alpha_ld att_enc att_dec wf B n P A E dalpha_ws dgp de dad stream
    ok = [q, 1, 0, q, q, q, q, 3, q, q, q, 2, 2, 3, 4, 4, q, q, q, q, None]
    fn = capmi.lib.capmi_att_group_bwd
    for hole in (0, 3, 4, 5, 6, 8, 9, 10, 16, 17, 18, 19):  # every pointer, the four outputs last
        a = list(ok)
        a[hole] = None
        assert fn(*a) == 1001, hole
    for pos, bad in ((12, 0), (12, 17), (12, -1), (11, 0), (13, 0), (14, 0), (15, 0), (1, 0), (7, 2)):
        a = list(ok)
        a[pos] = bad
        assert fn(*a) == 1001, (pos, bad)
    for pos, bad in ((14, 6), (15, 6), (2, 6), (11, 65536)):  # A % 4, E % 4, slab % 4, B
        a = list(ok)
        a[pos] = bad
        assert fn(*a) == 1003, (pos, bad)
    a = list(ok)
    a[12], a[15] = 16, 4096  # 16 rows of d(awe) at E = 4096 are 256 KiB: more than a CU's LDS
    assert fn(*a) == 1003
    a = list(ok)
    a[3] = q + 4
    assert fn(*a) == 1002
    del raw


def test_att_group_enc_grad_rejects_bad_arguments_before_any_launch():
    import capmi
    raw, q = _buf()
    nblk = ctypes.c_int(-5)
    # de att_enc att_dec wf T B n P A datt_enc wf_part bf_part nblk_out stream
    ok = [q, q, q, q, 2, 2, 2, 3, 4, q, q, q, ctypes.byref(nblk), None]
    fn = capmi.lib.capmi_att_group_enc_grad
    for hole in (0, 1, 2, 3, 9, 10, 11):
        a = list(ok)
        a[hole] = None
        assert fn(*a) == 1001, hole
    for pos, bad in ((6, 0), (6, 17), (4, 0), (5, 0), (7, 0), (8, 0)):
        a = list(ok)
        a[pos] = bad
        assert fn(*a) == 1001, (pos, bad)
    for pos, bad in ((8, 6), (8, 1028), (5, 65536)):  # A % 4, A / 4 > 256, B
        a = list(ok)
        a[pos] = bad
        assert fn(*a) == 1003, (pos, bad)
    assert nblk.value == -5  # a rejected call reports nothing
    del raw


def test_staging_plan_fits_whatever_T_and_n():
    """The (t, j) pairs of a group are staged in chunks: the kernel's LDS does not grow with T n."""
    for T, n, A in ((26, 16, 512), (26, 16, 1024), (1, 1, 4), (63, 16, 4)):
        ch, lds = GC.enc_grad_chunk(T, n, A)
        assert 1 <= ch <= min(T * n, 64) and ch * A <= 8192 and lds <= 55 * 1024 + 512, (T, n, A, ch, lds)
    assert GC.enc_grad_chunk(26, 16, 512) == (16, (16 * 512 + 16 * 28 + 4096) * 4)
    assert 26 * 16 * 512 * 4 > 160 * 1024  # what parking the whole group would take
    assert (26, 1, 16, 29, 512) in GC.GROUP_ENCGRAD_CASES


@pytest.mark.parametrize("case", GC.GROUP_BWD_CASES[:3] + GC.GROUP_BWD_CASES[4:], ids=DC.case_id)
def test_group_bwd_reference_is_the_replicated_reference(case):
    B, n, P, A, E, S = case
    p = GC.group_bwd_inputs(case)
    assert p["alpha"].stride(0) == 3 * P and p["enc"].shape == (B, P, E) and p["gate"].shape == (B * n, E)
    ref, direct = GC.group_bwd_ref(p, n), GC.group_bwd_direct(p, n)
    for k in ("dgp", "dalpha", "de", "dad"):
        val, mag = ref[k]
        assert val.dtype == torch.float64 and bool((mag >= 0).all())
        # both fp64: only the order of the sums separates them
        assert bool(((val - direct[k]).abs() <= 1e-12 * (mag + 1)).all()), k
    if P > 1:  # (a softmax over one slot has no gradient)
        assert float(ref["dad"][0].abs().max()) > 0 and float(ref["de"][0].abs().max()) > 0


def test_group_bwd_cases_cover_the_arms():
    ns = sorted(c[1] for c in GC.GROUP_BWD_CASES)
    assert ns == [1, 2, 4, 5, 16]  # the 4-arm partly full and full, the 8-arm, the 16-arm full
    assert any(c[2] % 13 for c in GC.GROUP_BWD_CASES) and any(c[3] % 64 for c in GC.GROUP_BWD_CASES)
    assert max(c[1] * c[4] * 4 for c in GC.GROUP_BWD_CASES) == 128 * 1024  # beyond the default 64 KiB of LDS


@pytest.mark.parametrize("case", [c for c in GC.GROUP_ENCGRAD_CASES if c[0] * c[2] <= 15], ids=DC.case_id)
def test_group_encgrad_reference_is_the_replicated_reference(case):
    T, B, n, P, A = case
    p = GC.group_encgrad_inputs(case)
    ref, direct = GC.group_encgrad_ref(p, n), GC.group_encgrad_direct(p, n)
    for k in ("datt_enc", "wf_grad", "bf_grad"):
        val, mag = ref[k]
        assert val.shape == direct[k].shape
        assert bool(((val - direct[k]).abs() <= 1e-12 * (mag + 1)).all()), k


def test_train_py_does_not_dispatch_to_the_attention_step_yet():
    """The two-line dispatch in train.py comes with the test that pins its refusal (tests/test_scst_cpu.py)."""
    import models.attention as MA
    import models.baseline as MB
    import types
    assert callable(MA.train_self_critical) and "train_self_critical" in MA.__all__
    args = types.SimpleNamespace(model="attention", self_critical=True)
    with pytest.raises(NotImplementedError):
        MB.check_self_critical_args(args)
