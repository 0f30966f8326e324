"""GPU: the decoder's non-GEMM kernels (csrc/decoder.hip, its loss in csrc/loss.hip, the fused attention pair of
csrc/decoder_step.hip, csrc/optim.hip), each against a plain fp64 reference of the same operation at the shapes where its code takes
another path: every arm of slab_sum, tail chunks along P, column tails along A and E, every leading stride
different from the row length, bt = 0 / some / all rows, each optional output present and absent.

Cases, references and comparison rules live in tests/decoder_kernel_cases.py (pinned themselves by
tests/test_decoder_kernel_cases_cpu.py); the references run in fp64 on the device from the very fp32 tensors the
kernel gets. Every input and output is a view into a NaN-filled buffer with 64-element guard zones on both
sides, strided views with NaN between their rows: an over-read reaches the result, and after the call the
guards and the gaps are still NaN and the output holds none."""
import math

import pytest
import torch

import decoder_kernel_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
GUARD = 64


def _K():
    from capmi import kernels as K
    return K


def gin(t):
    """An input on the device between two NaN guard zones. A strided view (DC.padded) is uploaded with its whole
    NaN-filled base, so the gaps between its rows are NaN on the device too."""
    if t is None:
        return None
    if not t.is_floating_point():
        return t.to(DEV)
    base = t if t._base is None else t._base
    n = base.numel()
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=t.dtype, device=DEV)
    buf[GUARD:GUARD + n] = base.reshape(-1).to(DEV)
    v = buf.as_strided(t.shape, t.stride(), GUARD + t.storage_offset())
    assert v.data_ptr() % 16 == 0
    return v


def dev(p):
    return {k: gin(v) if torch.is_tensor(v) else v for k, v in p.items()}


class Out:
    """An output of ``shape`` (rows..., cols) whose rows are ``ld`` apart (default: cols), in a NaN-filled buffer
    with guard zones; ``init`` gives an in-out buffer its values."""

    def __init__(self, shape, ld=None, dtype=F32, init=None):
        self.shape, self.cols = tuple(shape), shape[-1]
        self.rows, self.ld = math.prod(shape[:-1]), ld or shape[-1]
        self.buf = torch.full((self.rows * self.ld + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
        self.body = self.buf[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)
        self.v = self.body[:, :self.cols]
        if self.ld == self.cols:
            self.v = self.v.view(self.shape)
        if init is not None:
            self.v.copy_(init.reshape(self.v.shape))
        assert self.v.data_ptr() % 16 == 0

    def check(self, what):
        torch.cuda.synchronize()
        n = self.rows * self.ld
        assert bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + n:]).all()), \
            f"{what}: wrote outside its output"
        assert bool(torch.isnan(self.body[:, self.cols:]).all()), f"{what}: wrote between its rows"
        assert not bool(torch.isnan(self.v).any()), f"{what}: left part of its output unwritten (or wrote NaN)"
        return self.v.reshape(self.shape)

    def untouched(self, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf).all()), f"{what}: wrote although it rejected the call"


def slab(parts):
    return 0 if parts is None else parts.stride(0)


def nslab(parts):
    return 0 if parts is None else parts.shape[0]


def checked(outs, kernel):
    return {k: o.check(f"{kernel} {k}") for k, o in outs.items() if o is not None}


def v(o):
    return None if o is None else o.v


# ============================================================================================ part A
@pytest.mark.parametrize("case", DC.MEAN_CASES, ids=DC.case_id)
def test_mean_rows(case):
    B, P, E = case
    p = dev(DC.mean_inputs(case))
    out = Out((B, E))
    _K().mean_rows(p["enc"], B, P, E, out.v)
    DC.mean_compare({"mean": out.check("mean_rows")}, DC.mean_ref(p), f"mean_rows {case}")


@pytest.mark.parametrize("case", DC.SCORE_CASES, ids=DC.case_id)
def test_att_score_fwd(case):
    B, P, A, S, _, _, adout = case
    p = dev(DC.score_inputs(case))
    outs = dict(e=Out((B, P)), att_dec=Out((B, A)) if adout else None)
    _K().att_score_fwd(p["att_enc"], p["parts"], S, slab(p["parts"]), p["bias_da"], p["wf"], p["bf"], B, P, A, outs["e"].v,
                       v(outs["att_dec"]))
    DC.score_compare(checked(outs, "att_score_fwd"), DC.score_ref(p), S, f"att_score_fwd {DC.case_id(case)}")


@pytest.mark.parametrize("case", DC.SOFTCTX_CASES, ids=DC.case_id)
def test_att_softmax_ctx_fwd(case):
    B, P, E, bt, S, gate_out, x_out, awe_out = case
    p = dev(DC.softctx_inputs(case))
    outs = dict(alpha=Out((B, P), ld=3 * P), awe=Out((B, E)) if awe_out else None, gate=Out((B, E)) if gate_out else None,
                x=Out((B, E), ld=E + 12) if x_out else None)
    _K().att_softmax_ctx_fwd(p["e"], p["enc"], B, P, E, bt, outs["alpha"].v, 3 * P, v(outs["awe"]), p["gate_parts"], S,
                             slab(p["gate_parts"]), p["bias_fb"], v(outs["gate"]), v(outs["x"]), E + 12)
    DC.softctx_compare(checked(outs, "att_softmax_ctx_fwd"), DC.softctx_ref(p, bt), bt,
                       f"att_softmax_ctx_fwd {DC.case_id(case)}")


@pytest.mark.parametrize("case", DC.FWDF_CASES, ids=DC.case_id)
def test_att_fwd_fused(case):
    B, P, A, E, S_a, S_g, bt, ad_out, gate_out, awe_out, alpha_out = case
    p = dev(DC.fwdf_inputs(case))
    outs = dict(ad=Out((B, A)) if ad_out else None, gate=Out((B, E)) if gate_out else None, awe=Out((B, E)) if awe_out else None,
                alpha=Out((B, P), ld=3 * P) if alpha_out else None, x=Out((B, E), ld=E + 12))
    ad, gate = (p["ad_parts"] if S_a else p["ad"]), (p["gate_parts"] if S_g else p["gate"])
    _K().att_fwd_fused(p["att_enc"], ad, S_a, slab(ad) if S_a else 0, p.get("bias_da"), v(outs["ad"]), p["wf"], p["bf"], p["enc"],
                       gate, S_g, slab(gate) if S_g else 0, p.get("bias_fb"), v(outs["gate"]), B, P, A, E, bt, v(outs["alpha"]),
                       3 * P, v(outs["awe"]), outs["x"].v, E + 12)
    DC.fwdf_compare(checked(outs, "att_fwd_fused"), DC.fwdf_ref(p, bt), p, bt, f"att_fwd_fused {DC.case_id(case)}")


def run_ctx_bwd(p, B, P, E, gm, dawe_out):
    outs = dict(dgp=Out((B, E)) if gm == 1 else None, dalpha=Out((B, P)), dawe=Out((B, E)) if dawe_out else None)
    _K().att_ctx_bwd(p["parts"], nslab(p["parts"]), slab(p["parts"]), p["gate"], p["awe"], p["enc"], B, P, E, v(outs["dgp"]),
                     outs["dalpha"].v, v(outs["dawe"]))
    return checked(outs, "att_ctx_bwd")


@pytest.mark.parametrize("case", DC.CTXB_CASES, ids=DC.case_id)
def test_att_ctx_bwd(case):
    B, P, E, S, gm, dawe_out = case
    p = dev(DC.ctxb_inputs(case))
    DC.ctxb_compare(run_ctx_bwd(p, B, P, E, gm, dawe_out), DC.ctxb_ref(p), f"att_ctx_bwd {DC.case_id(case)}")


def run_score_bwd(p, dalpha, B, P, A, bt):
    outs = dict(de=Out((B, P)), dad=Out((B, A)))
    dreg = p["dreg"]
    _K().att_score_bwd(dalpha, dreg, 0 if dreg is None else dreg.stride(0), p["alpha"], p["alpha"].stride(0), p["att_enc"],
                       p["att_dec"], p["wf"], B, P, A, bt, outs["de"].v, outs["dad"].v)
    return checked(outs, "att_score_bwd")


@pytest.mark.parametrize("case", DC.SCOREB_CASES, ids=DC.case_id)
def test_att_score_bwd(case):
    B, P, A, bt, _ = case
    p = dev(DC.scoreb_inputs(case))
    assert p["alpha"].stride(0) == 3 * P and (p["dreg"] is None or p["dreg"].stride(0) == P + 8)
    DC.scoreb_compare(run_score_bwd(p, p["dalpha"], B, P, A, bt), DC.scoreb_ref(p, bt), bt, f"att_score_bwd {DC.case_id(case)}")


def run_bwd_fused(p, case):
    B, P, A, E, S, gm, bt, _, dawe_out = case
    outs = dict(dgp=Out((B, E)) if gm == 1 else None, dawe=Out((B, E)) if dawe_out else None, de=Out((B, P)), dad=Out((B, A)))
    dreg = p["dreg"]
    _K().att_bwd_fused(p["parts"], S, slab(p["parts"]), p["gate"], p["awe"], v(outs["dgp"]), v(outs["dawe"]), p["enc"], p["alpha"],
                       p["alpha"].stride(0), dreg, 0 if dreg is None else dreg.stride(0), p["att_enc"], p["att_dec"], p["wf"],
                       B, P, A, E, bt, outs["de"].v, outs["dad"].v)
    return checked(outs, "att_bwd_fused")


@pytest.mark.parametrize("case", DC.BWDF_CASES, ids=DC.case_id)
def test_att_bwd_fused(case):
    p = dev(DC.bwdf_inputs(case))
    bt = case[6]
    DC.bwdf_compare(run_bwd_fused(p, case), DC.bwdf_ref(p, bt), bt, f"att_bwd_fused {DC.case_id(case)}")


@pytest.mark.parametrize("case", DC.BWDF_IDENTITY_CASES, ids=DC.case_id)
def test_att_bwd_fused_is_the_two_kernels_bit_for_bit(case):
    """csrc/decoder_step.hip states that att_bwd_fused is bit-identical to att_ctx_bwd followed by att_score_bwd."""
    B, P, A, E, S, gm, bt, _, dawe_out = case
    assert (A, S, gm) == (260, 5, 1)
    p = dev(DC.bwdf_inputs(case))
    fused = run_bwd_fused(p, case)
    two = run_ctx_bwd(p, B, P, E, gm, dawe_out)
    two.update(run_score_bwd(p, two.pop("dalpha"), B, P, A, bt))
    for k in ("dgp", "dawe", "de", "dad"):
        DC.exact(fused[k], two[k], f"att_bwd_fused {DC.case_id(case)} {k} against the two kernels")


@pytest.mark.parametrize("case", DC.DINPUT_CASES, ids=DC.case_id)
def test_att_enc_dinput(case):
    B, P, T, E, _ = case
    p = dev(DC.dinput_inputs(case))
    assert p["alpha"].stride(0) == T * P + 4
    out = Out((B, P, E))
    _K().att_enc_dinput(p["alpha"], T * P + 4, p["dawe"], p["dmean"], B, T, P, E, out.v)
    DC.dinput_compare({"denc": out.check("att_enc_dinput")}, DC.dinput_ref(p), f"att_enc_dinput {DC.case_id(case)}")


@pytest.mark.parametrize("case", DC.ENCGRAD_CASES, ids=DC.case_id)
def test_att_enc_grad(case):
    """datt_enc element-wise; wf_part and bf_part summed over the nblk workgroups the call reports. The last case
    needs more than 64 KiB of dynamic LDS."""
    K = _K()
    B, P, T, A = case
    p = dev(DC.encgrad_inputs(case))
    nblk = K.att_enc_grad_blocks(B, P)
    assert nblk == DC.chunks(P, DC.PCH)[0] * B
    outs = dict(datt_enc=Out((B, P, A)), wf_part=Out((nblk, A)), bf_part=Out((nblk,)))
    assert K.att_enc_grad(p["de"], p["att_enc"], p["att_dec"], p["wf"], T, B, P, A, outs["datt_enc"].v, outs["wf_part"].v,
                          outs["bf_part"].v) == nblk
    got = checked(outs, "att_enc_grad")
    got = dict(datt_enc=got["datt_enc"], wf_grad=got["wf_part"].double().sum(0), bf_grad=got["bf_part"].double().sum())
    DC.encgrad_compare(got, DC.encgrad_ref(p), f"att_enc_grad {DC.case_id(case)}")


# ============================================================================================ part B
@pytest.mark.parametrize("case", DC.LSTM_FWD_CASES, ids=DC.case_id)
def test_lstm_cell_fwd(case):
    B, D, S, S2, _ = case
    p = dev(DC.lstm_fwd_inputs(case))
    outs = dict(h=Out((B, D)), c=Out((B, D)), act=Out((B, 4 * D)))
    _K().lstm_cell_fwd(p["parts"], S, slab(p["parts"]), p["xemb"], p["hh_parts"], S2, slab(p["hh_parts"]), p["c_prev"], B, D,
                       outs["h"].v, outs["c"].v, outs["act"].v)
    DC.lstm_fwd_compare(checked(outs, "lstm_cell_fwd"), DC.lstm_fwd_ref(p), f"lstm_cell_fwd {DC.case_id(case)}")


@pytest.mark.parametrize("case", DC.LSTM_BWD_CASES, ids=DC.case_id)
def test_lstm_cell_bwd(case):
    B, D, bt, _, _, S = case
    p = dev(DC.lstm_bwd_inputs(case))
    outs = dict(dgates=Out((B, 4 * D)), dc_out=Out((B, D)))
    _K().lstm_cell_bwd(p["dhd"], p["dh_parts"], S, slab(p["dh_parts"]), p["dc_in"], p["act"], p["c_prev"], p["c_cur"], B, D, bt,
                       outs["dgates"].v, outs["dc_out"].v)
    DC.lstm_bwd_compare(checked(outs, "lstm_cell_bwd"), DC.lstm_bwd_ref(p, bt), bt, f"lstm_cell_bwd {DC.case_id(case)}")


@pytest.mark.parametrize("case", DC.CE_CASES, ids=DC.case_id)
def test_ce_fwd_bwd(case):
    V, _, tm, _, lse, dl = case
    B, T, L = DC.CE_B, DC.CE_T, DC.CE_L
    p = dev(DC.ce_inputs(case))
    outs = dict(loss=Out((B, T)), lse=Out((B, T)) if lse else None, dlogits=Out((B * T, V)) if dl else None)
    _K().ce_fwd_bwd(p["logits"], p["caps"], B, T, L, V, p["bt"], p["nrows"], outs["loss"].v, v(outs["lse"]), v(outs["dlogits"]),
                    dl_time_major=bool(tm), gscale=p["gscale"])
    DC.ce_compare(checked(outs, "ce_fwd_bwd"), DC.ce_ref(p), f"ce_fwd_bwd {DC.case_id(case)}")


@pytest.mark.parametrize("V", [7, 257])
def test_ce_fwd_bwd_never_follows_a_target_outside_the_vocabulary(V):
    """Live rows (0, 0) and (1, 1) with targets V and -1: zero loss, zero lse and a zero gradient row, as
    capmi_ce_ignore_fwd_bwd and capmi_pg_ce_fwd_bwd treat them; every other row is bit-equal to the same call
    with valid targets in those two positions."""
    B, T, L = DC.CE_B, DC.CE_T, DC.CE_L
    p = dev(DC.ce_inputs((V, 1, 0, 1, 1, 1)))
    bad = p["caps"].clone()
    bad[0, 1], bad[1, 2] = V, -1
    got = {}
    for name, caps in (("valid", p["caps"]), ("outside", bad)):
        outs = dict(loss=Out((B, T)), lse=Out((B, T)), dlogits=Out((B * T, V)))
        _K().ce_fwd_bwd(p["logits"], caps, B, T, L, V, p["bt"], p["nrows"], outs["loss"].v, outs["lse"].v, outs["dlogits"].v,
                        gscale=p["gscale"])
        got[name] = checked(outs, f"ce_fwd_bwd {name} targets")
    rows = torch.tensor([0 * T + 0, 1 * T + 1], device=DEV)
    rest = torch.ones(B * T, dtype=torch.bool, device=DEV)
    rest[rows] = False
    for k, o in got["outside"].items():
        o, ref = o.reshape(B * T, -1), got["valid"][k].reshape(B * T, -1)
        assert bool((o[rows].view(torch.int32) == 0).all()), f"{k} of a row whose target is outside [0, V)"
        assert bool((ref[rows] != 0).any(1).all()), f"{k}: the rows under test are live with valid targets"
        DC.exact(o[rest], ref[rest], f"{k} of the other rows")


@pytest.mark.parametrize("case", DC.REG_CASES, ids=DC.case_id)
def test_alpha_reg(case):
    K = _K()
    B, T, P, dreg = case
    p = dev(DC.reg_inputs(case))
    nblk = K.alpha_reg_parts(B, P)
    assert nblk == DC.chunks(B * P, 256)[0]
    outs = dict(reg_part=Out((nblk,)), dreg=Out((B, P)) if dreg else None)
    K.alpha_reg(p["alphas"], B, T, P, DC.ALPHA_C, outs["reg_part"].v, v(outs["dreg"]))
    got = checked(outs, "alpha_reg")
    got["reg"] = got.pop("reg_part").double().sum()
    DC.reg_compare(got, DC.reg_ref(p), f"alpha_reg {DC.case_id(case)}")


@pytest.mark.parametrize("case", DC.LOSSFIN_CASES, ids=DC.case_id)
def test_loss_finalize(case):
    p = dev(DC.lossfin_inputs(case))
    out = Out((1,))
    _K().loss_finalize(p["rows"], case[0], p["nrows"], p["reg"], out.v)
    DC.within(out.check("loss_finalize"), *DC.lossfin_ref(p)["loss"], f"loss_finalize {case}")


@pytest.mark.parametrize("case", DC.GATHER_CASES, ids=DC.case_id)
def test_embed_gather(case):
    M = case[1]
    p = dev(DC.gather_inputs(case))
    out = Out((DC.EMB_T, DC.EMB_B, M), ld=M + 8)
    _K().embed_gather(p["emb"], p["caps"], DC.EMB_B, DC.EMB_L, DC.EMB_T, out.v, M + 8)
    DC.exact(out.check("embed_gather"), DC.gather_ref(p), f"embed_gather {case}")


@pytest.mark.parametrize("case", DC.DENSE_CASES, ids=DC.case_id)
def test_embed_dense(case):
    B, Le, M, T = case
    p = dev(DC.dense_inputs(case))
    out = Out((T, B, M), ld=M + 8)
    _K().embed_dense(p["emb"], T, out.v, M + 8)
    DC.exact(out.check("embed_dense"), DC.dense_ref(p, T), f"embed_dense {case}")


@pytest.mark.parametrize("remap", [0, 1])
def test_mask_rows_tb(remap):
    """plain: x is (T, B, cols) rows ld apart; two-level remap (r1 = B, s2 = cols): x is (B, T, cols) with the
    batch rows ld apart"""
    T, B, cols = DC.MASK_T, DC.MASK_B, DC.MASK_COLS
    x = DC._u(DC.gen("mask", (remap,)), (T, B, cols)) + 1.5  # (no zero among the kept values)
    bt = torch.tensor(DC.MASK_BT, dtype=torch.int32, device=DEV)
    if remap:
        ld = T * cols + 4
        buf = Out((B, T * cols), ld=ld, init=x.transpose(0, 1).reshape(B, T * cols).to(DEV))
        _K().mask_rows_tb(buf.v, bt, T, B, cols, ld, r1=B, s2=cols)
        got = buf.check("mask_rows_tb").view(B, T, cols).transpose(0, 1)
    else:
        ld = cols + 3
        buf = Out((T, B, cols), ld=ld, init=x.to(DEV))
        _K().mask_rows_tb(buf.v, bt, T, B, cols, ld)
        got = buf.check("mask_rows_tb")
    DC.exact(got.contiguous(), DC.mask_ref(x).to(DEV), f"mask_rows_tb remap {remap}")


def test_dropout():
    K = _K()
    n = DC.DROPOUT_N
    x = gin(DC._u(DC.gen("dropout", (n,)), (n,)) + 1.5)
    out = Out((n,))
    K.dropout(x, n, 0.0, 1234, out.v)
    DC.exact(out.check("dropout p=0"), x, "dropout p = 0 is the identity")
    a, b, c = Out((n,)), Out((n,)), Out((n,))
    K.dropout(x, n, 0.5, 1234, a.v)
    K.dropout(x, n, 0.5, 1234, b.v)
    K.dropout(x, n, 0.5, 1235, c.v)
    a, b, c = a.check("dropout"), b.check("dropout"), c.check("dropout")
    DC.exact(b, a, "dropout with the same seed")
    kept = a != 0
    DC.exact(a[kept], (2 * x)[kept], "dropout p = 0.5 kept elements")
    frac = float(kept.double().mean())
    print(f"dropout keep fraction {frac:.4f}")
    assert abs(frac - 0.5) <= 0.01, frac
    assert 0.4 < float(((c != 0) != kept).double().mean()) < 0.6  # another seed, another mask


# ============================================================================================ part C
HYPER = (DC.ADAM["lr"], DC.ADAM["beta1"], DC.ADAM["beta2"], DC.ADAM["eps"])


@pytest.mark.parametrize("case", DC.ADAM_CASES, ids=DC.case_id)
def test_adam_clamp(case):
    """Three steps from non-zero moments, each against the fp64 restatement fed the state the kernel got; then the
    same three steps with the device step counter, bit-equal to the host-computed bias corrections."""
    K = _K()
    T, n = DC.adam_dtype(case), case[1]
    s = DC.adam_inputs(case, DEV)
    grads = [gin(g) for g in s["g"]]
    st = {k: Out((n,), dtype=T, init=s[k]) for k in "pmv"}
    host = []
    for step in range(1, DC.ADAM_STEPS + 1):
        before = {k: st[k].v.clone() for k in "pmv"}
        bc1, bc2s = DC.adam_bc(step)
        K.adam_clamp(st["p"].v, grads[step - 1], st["m"].v, st["v"].v, *HYPER, bc1, bc2s, DC.ADAM["clip"])
        got = {k: st[k].check(f"adam_clamp {k}") for k in "pmv"}
        ref = DC.adam_ref(before["p"], grads[step - 1], before["m"], before["v"], step, T)
        DC.adam_compare(got, ref, T, f"adam_clamp {case[0]} n={n}")
        host.append({k: got[k].clone() for k in "pmv"})
        del ref, before
    st = {k: Out((n,), dtype=T, init=s[k]) for k in "pmv"}
    counter = torch.ones(1, dtype=torch.int64, device=DEV)
    for step in range(1, DC.ADAM_STEPS + 1):
        K.adam_clamp(st["p"].v, grads[step - 1], st["m"].v, st["v"].v, *HYPER, 1.0, 1.0, DC.ADAM["clip"], step_dev=counter)
        K.counter_add(counter)
        for k in "pmv":
            DC.exact(st[k].check(f"adam_clamp {k}"), host[step - 1][k], f"adam_clamp {case[0]} n={n} device step {step} {k}")
    assert int(counter) == DC.ADAM_STEPS + 1


@pytest.mark.parametrize("case", DC.SCATTER_CASES, ids=DC.case_id)
def test_embed_scatter_add(case):
    p = dev(DC.scatter_inputs(case))
    assert p["dx"].stride(1) == DC.SC_M + 4
    demb = Out((DC.SC_V, DC.SC_M), dtype=p["demb"].dtype, init=p["demb"])
    _K().embed_scatter_add(p["dx"], DC.SC_M + 4, p["caps"], DC.SC_B, DC.SC_L, DC.SC_T, p["bt"], DC.SC_M, demb.v)
    DC.scatter_compare(demb.check("embed_scatter_add"), DC.scatter_ref(p), p["demb"], f"embed_scatter_add {DC.case_id(case)}")


# ============================================================================================ rejections
def rejected(what, outs, fn, *a, **kw):
    from capmi import CapmiError
    with pytest.raises(CapmiError):
        fn(*a, **kw)
    for o in outs:
        o.untouched(what)


def test_argument_rejections():
    """The wrappers refuse before any launch: the call raises CapmiError and the NaN-filled outputs stay NaN. Every
    tensor is a stand-in of valid size, so a check that ever regressed would launch on good pointers."""
    K = _K()
    B, P, A, E = 2, 8, 8, 8
    f = lambda *shape: torch.ones(*shape, device=DEV)  # noqa: E731

    def off(*shape):  # a view one float past a 16-byte boundary
        n = math.prod(shape)
        t = torch.ones(n + 4, device=DEV)[1:1 + n].view(*shape)
        assert t.data_ptr() % 16 == 4
        return t

    e, ad = Out((B, P)), Out((B, A))
    rejected("att_score_fwd A=6", [e, ad], K.att_score_fwd, f(B, P, A), f(1, B * A), 1, B * A, f(A), f(A), f(1), B, P, 6, e.v, ad.v)
    rejected("att_score_fwd misaligned att_enc", [e, ad], K.att_score_fwd, off(B, P, A), f(1, B * A), 1, B * A, f(A), f(A), f(1),
             B, P, A, e.v, ad.v)
    x, alpha = Out((B, E)), Out((B, 57))
    rejected("att_fwd_fused P=57", [x, alpha], K.att_fwd_fused, f(B, 57, A), f(B, A), 0, 0, None, None, f(A), f(1), f(B, 57, E),
             f(B, E), 0, 0, None, None, B, 57, A, E, B, alpha.v, 57, None, x.v, E)
    rejected("att_fwd_fused A=6", [x, alpha], K.att_fwd_fused, f(B, P, A), f(B, A), 0, 0, None, None, f(A), f(1), f(B, P, E),
             f(B, E), 0, 0, None, None, B, P, 6, E, B, alpha.v, 57, None, x.v, E)
    rejected("att_fwd_fused misaligned enc", [x, alpha], K.att_fwd_fused, f(B, P, A), f(B, A), 0, 0, None, None, f(A), f(1),
             off(B, P, E), f(B, E), 0, 0, None, None, B, P, A, E, B, alpha.v, 57, None, x.v, E)
    big = 1028
    dx, wfp, bfp = Out((B, P, big)), Out((B, big)), Out((B,))
    rejected("att_enc_grad A=1028", [dx, wfp, bfp], K.att_enc_grad, f(1, B, P), f(B, P, big), f(1, B, big), f(big), 1, B, P, big,
             dx.v, wfp.v, bfp.v)
    dal, dgp = Out((B, P)), Out((B, E))
    rejected("att_ctx_bwd misaligned enc", [dal, dgp], K.att_ctx_bwd, f(1, B * E), 1, B * E, f(B, E), f(B, E), off(B, P, E), B, P, E,
             dgp.v, dal.v)
    rejected("att_ctx_bwd dgp without gate", [dal, dgp], K.att_ctx_bwd, f(1, B * E), 1, B * E, None, None, f(B, P, E), B, P, E,
             dgp.v, dal.v)
    de, dad = Out((B, P)), Out((B, A))
    rejected("att_score_bwd A=6", [de, dad], K.att_score_bwd, f(B, P), None, 0, f(B, P), P, f(B, P, A), f(B, A), f(A), B, P, 6, B,
             de.v, dad.v)
    rejected("att_bwd_fused misaligned att_dec", [de, dad], K.att_bwd_fused, f(1, B * E), 1, B * E, None, None, None, None,
             f(B, P, E), f(B, P), P, None, 0, f(B, P, A), off(B, A), f(A), B, P, A, E, B, de.v, dad.v)
    m = Out((B, E))
    rejected("mean_rows misaligned enc", [m], K.mean_rows, off(B, P, E), B, P, E, m.v)
    rejected("mean_rows E=6", [m], K.mean_rows, f(B, P, E), B, P, 6, m.v)
    pm = {k: Out((16,), init=f(16)) for k in "pmv"}
    from capmi import CapmiError
    with pytest.raises(CapmiError):  # neither a step counter nor positive bias corrections
        K.adam_clamp(pm["p"].v, f(16), pm["m"].v, pm["v"].v, *HYPER, 0.0, 0.0, DC.ADAM["clip"])
    for k in "pmv":
        DC.exact(pm[k].check(f"adam_clamp {k}"), f(16), f"adam_clamp rejected: {k} unchanged")
