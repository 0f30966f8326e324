"""GPU: the grouped attention-backward kernels of csrc/att_group.hip (capmi_att_group_bwd,
capmi_att_group_enc_grad) against the fp64 references of tests/decoder_kernel_cases.py applied to features
replicated per row (tests/att_group_cases.py, pinned by tests/test_scst_attention_cpu.py). Inputs and outputs
live in NaN-filled buffers with guard zones (the harness of tests/test_gpu_decoder_kernels.py): an over-read
reaches the result, and nothing outside the documented extents may be written."""
import pytest
import torch

import att_group_cases as GC
import decoder_kernel_cases as DC
from test_gpu_decoder_kernels import Out, checked, dev, nslab, slab

pytestmark = pytest.mark.gpu


def _K():
    from capmi import kernels as K
    return K


def run_group_bwd(p, B, n, P, A, E):
    R = B * n
    outs = dict(dalpha=Out((R, P)), dgp=Out((R, E)), de=Out((R, P)), dad=Out((R, A)))
    _K().att_group_bwd(p["parts"], nslab(p["parts"]), slab(p["parts"]), p["gate"], p["awe"], p["enc"], p["alpha"],
                       p["alpha"].stride(0), p["att_enc"], p["att_dec"], p["wf"], B, n, P, A, E, outs["dalpha"].v,
                       outs["dgp"].v, outs["de"].v, outs["dad"].v)
    return checked(outs, "att_group_bwd")


@pytest.mark.parametrize("case", GC.GROUP_BWD_CASES, ids=DC.case_id)
def test_att_group_bwd(case):
    B, n, P, A, E, S = case
    p = dev(GC.group_bwd_inputs(case))
    assert p["alpha"].stride(0) == 3 * P and nslab(p["parts"]) == S
    GC.group_bwd_compare(run_group_bwd(p, B, n, P, A, E), GC.group_bwd_ref(p, n), S, f"att_group_bwd {DC.case_id(case)}")


def test_a_row_computes_the_same_bits_alone_and_in_a_group():
    """Every row of the n = 5 case again as its own image (n = 1, the 4-row arm instead of the 8-row one)."""
    case = GC.GROUP_BWD_IDENTITY_CASE
    B, n, P, A, E, S = case
    assert n == 5
    p = dev(GC.group_bwd_inputs(case))
    grouped = run_group_bwd(p, B, n, P, A, E)
    alone = dict(p, enc=GC.rep(p["enc"], n).contiguous(), att_enc=GC.rep(p["att_enc"], n).contiguous())
    single = run_group_bwd(alone, B * n, 1, P, A, E)
    for k in ("dalpha", "dgp", "de", "dad"):
        DC.exact(single[k], grouped[k], f"att_group_bwd {k}: a row alone against the row in its group")


@pytest.mark.parametrize("case", GC.GROUP_ENCGRAD_CASES, ids=DC.case_id)
def test_att_group_enc_grad(case):
    """datt_enc element-wise; wf_part and bf_part summed over the workgroups the call reports."""
    K = _K()
    T, B, n, P, A = case
    p = dev(GC.group_encgrad_inputs(case))
    nblk = K.att_enc_grad_blocks(B, P)
    assert GC.enc_grad_chunk(T, n, A)[1] <= 64 * 1024
    outs = dict(datt_enc=Out((B, P, A)), wf_part=Out((nblk, A)), bf_part=Out((nblk,)))
    assert K.att_group_enc_grad(p["de"], p["att_enc"], p["att_dec"], p["wf"], T, B, n, P, A, outs["datt_enc"].v,
                                outs["wf_part"].v, outs["bf_part"].v) == nblk
    got = checked(outs, "att_group_enc_grad")
    got = dict(datt_enc=got["datt_enc"], wf_grad=got["wf_part"].double().sum(0), bf_grad=got["bf_part"].double().sum())
    GC.group_encgrad_compare(got, GC.group_encgrad_ref(p, n), f"att_group_enc_grad {DC.case_id(case)}")


def test_grouped_enc_grad_of_single_rows_is_the_ungrouped_kernel_in_value():
    """n = 1 is capmi_att_enc_grad's problem: both kernels within the accumulation rule of the same reference."""
    K = _K()
    T, B, P, A = 3, 2, 29, 512
    p = dev(GC.group_encgrad_inputs((T, B, 1, P, A)))
    nblk = K.att_enc_grad_blocks(B, P)
    ref = DC.encgrad_ref(p)
    for name, call in (("grouped", lambda o: K.att_group_enc_grad(p["de"], p["att_enc"], p["att_dec"], p["wf"], T, B, 1, P, A, *o)),
                       ("ungrouped", lambda o: K.att_enc_grad(p["de"], p["att_enc"], p["att_dec"], p["wf"], T, B, P, A, *o))):
        outs = dict(datt_enc=Out((B, P, A)), wf_part=Out((nblk, A)), bf_part=Out((nblk,)))
        call([outs[k].v for k in ("datt_enc", "wf_part", "bf_part")])
        got = checked(outs, name)
        DC.encgrad_compare(dict(datt_enc=got["datt_enc"], wf_grad=got["wf_part"].double().sum(0),
                                bf_grad=got["bf_part"].double().sum()), ref, f"{name} enc_grad")


def test_rejected_calls_write_nothing():
    K = _K()
    case = GC.GROUP_BWD_CASES[1]
    B, n, P, A, E, S = case
    p = dev(GC.group_bwd_inputs(case))
    from capmi._lib import lib
    q = lambda t: t.data_ptr()  # noqa: E731
    for bad_n, bad_a, code in ((0, A, 1001), (17, A, 1001), (n, A + 2, 1003)):
        outs = dict(dalpha=Out((B * n, P)), dgp=Out((B * n, E)), de=Out((B * n, P)), dad=Out((B * n, A)))
        assert lib.capmi_att_group_bwd(q(p["parts"]), S, slab(p["parts"]), q(p["gate"]), q(p["awe"]), q(p["enc"]),
                                       q(p["alpha"]), 3 * P, q(p["att_enc"]), q(p["att_dec"]), q(p["wf"]), B, bad_n, P,
                                       bad_a, E, q(outs["dalpha"].v), q(outs["dgp"].v), q(outs["de"].v), q(outs["dad"].v),
                                       K.stream()) == code
        for k, o in outs.items():
            o.untouched(f"att_group_bwd n={bad_n} A={bad_a} {k}")
