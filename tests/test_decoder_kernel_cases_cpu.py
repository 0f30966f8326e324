"""CPU: the references and comparison rules of the decoder non-GEMM kernel tests
(tests/decoder_kernel_cases.py, which tests/test_gpu_decoder_kernels.py runs the kernels against).

  * the planned paths: which slab_sum arms each S takes, the chunk counts of each P, the p-groups and idle threads
    of each A, the dynamic LDS of the T = 40 case, and the ReLU masks agreeing between fp32 and fp64;
  * the references are anchored to fp64 autograd (relative L2 <= 1e-12): the attention forward and its backward
    chain, the LSTM cell, the cross entropy, the alpha regulariser, and Adam to torch.optim.Adam;
  * the bounds are reachable: the fp32 emulation of every case (the reference computed in fp32, slab sums in
    slab order) passes the very comparison the GPU test makes;
  * every rule has teeth: the emulation of a plausible kernel bug fails it."""
import math

import pytest
import torch

import decoder_kernel_cases as DC
from helpers import rel_err

F32, F64 = torch.float32, torch.float64


def emu(ref):
    """the outputs of a reference run in fp32, as a kernel would hand them over"""
    return {k: v[0].float() for k, v in ref.items() if isinstance(v, tuple)}


def fails(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


# ------------------------------------------------------------------------------------------ the planned paths
def test_planned_paths():
    arms = {S: DC.slab_arms(S) for S in (0, 1, 3, 4, 5, 8, 13)}
    assert arms == {0: (0, False, 0), 1: (0, False, 1), 3: (0, False, 3), 4: (0, True, 0), 5: (0, True, 1), 8: (1, False, 0),
                    13: (1, True, 1)}
    assert sorted({c[3] for c in DC.SCORE_CASES}) == [1, 3, 4, 8, 13]
    assert sorted({c[3] - 1 for c in DC.CTXB_CASES}) == [0, 1, 4, 8]  # att_ctx_bwd sums the slabs after the first
    assert sorted({c[4] for c in DC.SOFTCTX_CASES}) == [0, 1, 4, 13]
    assert [DC.chunks(P, DC.PCH_T) for P in (1, 13, 14, 29)] == [(1, 1), (1, 13), (2, 1), (3, 3)]
    assert [DC.chunks(P, DC.PCH) for P in (1, 28, 29)] == [(1, 1), (1, 28), (2, 1)]
    assert [DC.chunks(P, DC.DIN_PB) for P in (1, 8, 9, 29)] == [(1, 1), (1, 8), (2, 1), (4, 5)]
    assert [DC.enc_grad_plan(A) for A in (4, 48, 512, 1024)] == [(1, 256, 0), (12, 21, 4), (128, 2, 0), (256, 1, 0)]
    _, _, T, A = DC.ENCGRAD_BIG_LDS
    assert 64 * 1024 < DC.enc_grad_lds(T, A) == 90496 <= 160 * 1024
    assert all(DC.enc_grad_lds(c[2], c[3]) <= 64 * 1024 for c in DC.ENCGRAD_CASES[:-1])
    assert DC.enc_grad_lds(51, 512) == 114256  # a real caption length: 111.6 KiB
    assert DC.ADAM_N[-1] - 8192 * 256 == 3
    B, _, P, _ = DC.REG_CASES[2]
    assert DC.chunks(B * P, 256) == (4, 212)
    for c in DC.FWDF_CASES:
        assert c[1] <= 56
    for c in DC.BWDF_CASES:  # capmi_att_bwd_fused's LDS: E + P + 16 * 64 * 4 floats within 64 KiB
        assert (c[3] + ((c[1] + 3) & ~3) + 4096) * 4 <= 64 * 1024


def test_relu_masks_agree():
    """The sign of the fp32 sum att_enc + att_dec is the sign of the fp64 sum of the same inputs, in every element
    of every backward case: no kink is excused."""
    n = 0
    for cases, inputs in ((DC.SCOREB_CASES, DC.scoreb_inputs), (DC.BWDF_CASES, DC.bwdf_inputs),
                          (DC.ENCGRAD_CASES, DC.encgrad_inputs)):
        for c in cases:
            p = inputs(c)
            x, ad = p["att_enc"], p["att_dec"]
            s32 = x + (ad[:, None, :] if ad.dim() == 2 else ad[:, :, None, :])
            assert s32.dtype == F32
            m = DC.kink_mask(x, ad)
            assert bool(((s32 > 0) == m).all()), c
            assert m.numel() < 1000 or 0.3 < float(m.double().mean()) < 0.7  # both branches are taken
            n += m.numel()
    print(f"{n} mask elements agree")


# ------------------------------------------------------------------------------------------ a. the anchors
def test_attention_chain_is_autograd():
    """scores -> softmax -> context -> gate forward, and att_ctx_bwd -> att_score_bwd -> att_enc_grad +
    att_enc_dinput backward (one timestep), against autograd through SoftAttention's formula in fp64."""
    B, P, A, E = 3, 29, 68, 260
    g = DC.gen("anchor", (B, P, A, E))
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64) * 2 - 1  # noqa: E731
    att_enc, att_dec, wf, bf, enc, gpre, dx = r(B, P, A), r(B, A), r(A) * 0.2, r(1), r(B, P, E), r(B, E) * 4, r(B, E)
    leaves = [t.clone().requires_grad_() for t in (att_enc, att_dec, wf, bf, enc, gpre)]
    xe, xd, w, b0, en, gp = leaves
    e = torch.relu(xe + xd[:, None, :]) @ w + b0
    alpha = torch.softmax(e, 1)
    awe = (alpha[:, :, None] * en).sum(1)
    x = torch.sigmoid(gp) * awe
    x.backward(dx)
    # forward reference
    e_ref, _ = DC.scores(att_enc, att_dec, torch.zeros(B, A, dtype=F64), wf, bf, F64)
    gate = torch.sigmoid(gpre)
    f = DC.softmax_ctx(e_ref, None, enc, B, gate, torch.ones_like(gate), F64)
    errs = {"e": rel_err(e_ref, e), "alpha": rel_err(f["alpha"][0], alpha), "awe": rel_err(f["awe"][0], awe),
            "x": rel_err(f["x"][0], x)}
    # backward references, chained
    cb = DC.ctx_bwd(dx[None], gate, f["awe"][0], enc, F64)
    sb = DC.score_bwd(cb["dalpha"][0], cb["dalpha"][1], None, f["alpha"][0], att_enc, att_dec, wf, B, F64)
    eg = DC.encgrad_ref(dict(de=sb["de"][0][None], att_enc=att_enc, att_dec=att_dec[None], wf=wf))
    di = DC.dinput_ref(dict(alpha=f["alpha"][0][:, None, :], dawe=cb["dawe"][0][None], dmean=None))
    errs.update(dgp=rel_err(cb["dgp"][0], gp.grad), dad=rel_err(sb["dad"][0], xd.grad),
                datt_enc=rel_err(eg["datt_enc"][0], xe.grad), dwf=rel_err(eg["wf_grad"][0], w.grad),
                dbf=float((eg["bf_grad"][0] - b0.grad[0]).abs()),  # (a softmax backward sums to zero)
                denc=rel_err(di["denc"][0], en.grad))
    print("attention chain vs autograd:", {k: f"{v:.2g}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


def test_dmean_term_is_autograd():
    """att_enc_dinput's second term: the gradient of enc.mean(1) fed dmean"""
    B, P, E = 2, 9, 4
    p = DC.dinput_inputs((B, P, 4, E, 1))
    enc = torch.zeros(B, P, E, dtype=F64, requires_grad=True)
    enc.mean(1).backward(p["dmean"].double())
    only = DC.dinput_ref(dict(alpha=torch.zeros(B, 1, P), dawe=torch.zeros(1, B, E), dmean=p["dmean"]))
    assert rel_err(only["denc"][0], enc.grad) <= 1e-12


def test_lstm_cell_backward_is_autograd():
    B, D = 3, 5
    p = DC.lstm_fwd_inputs((B, D, 13, 4, 1))
    pre = DC.slab_total(p["hh_parts"], DC.slab_total(p["parts"], p["xemb"])[0])[0].clone().requires_grad_()
    cp = p["c_prev"].double().clone().requires_grad_()
    q = pre.view(B, 4, D)
    c = torch.sigmoid(q[:, 1]) * cp + torch.sigmoid(q[:, 0]) * torch.tanh(q[:, 2])
    h = torch.sigmoid(q[:, 3]) * torch.tanh(c)
    f = DC.lstm_fwd_ref(p)
    assert max(rel_err(f["c"][0], c), rel_err(f["h"][0], h)) <= 1e-12
    b = DC.lstm_bwd_inputs((B, D, B, 1, 1, 5))
    b.update(act=f["act"][0], c_cur=f["c"][0], c_prev=p["c_prev"])  # unrounded, so that autograd sees the same
    dh = DC.slab_total(b["dh_parts"], b["dhd"])[0]
    ((h * dh).sum() + (c * b["dc_in"].double()).sum()).backward()
    r = DC.lstm_bwd_ref(b, B)
    errs = rel_err(r["dgates"][0], pre.grad), rel_err(r["dc_out"][0], cp.grad)
    print("lstm cell backward vs autograd:", errs)
    assert max(errs) <= 1e-12, errs


def test_ce_and_alpha_reg_are_autograd():
    for case in (DC.CE_CASES[1], DC.CE_CASES[3]):
        p = DC.ce_inputs(case)
        r = DC.ce_ref(p)
        x = p["logits"].double().clone().requires_grad_()
        tgt = p["caps"][:, 1:DC.CE_T + 1]
        rows = torch.nn.functional.cross_entropy(x.view(-1, case[0]), tgt.reshape(-1), reduction="none").view(DC.CE_B, DC.CE_T)
        (rows * r["live"]).sum().backward()
        g = x.grad * (float(p["gscale"]) / p["nrows"])  # the fp32 device scalar
        if p["tm"]:
            g = g.transpose(0, 1)
        errs = rel_err(r["loss"][0], rows * r["live"]), rel_err(r["dlogits"][0], g.reshape(-1, case[0]))
        assert max(errs) <= 1e-12, errs
        assert p["nrows"] == int(r["live"].sum())
    p = DC.reg_inputs(DC.REG_CASES[1])
    a = p["alphas"].double().clone().requires_grad_()
    reg = ((DC.ALPHA_C - a.sum(1)) ** 2).mean()
    reg.backward()
    r = DC.reg_ref(p)
    errs = [rel_err(r["reg"][0], reg)] + [rel_err(r["dreg"][0], a.grad[:, t]) for t in range(a.shape[1])]
    assert max(errs) <= 1e-12, errs


def test_adam_reference_is_torch_adam():
    """Three steps of the reference, chained in fp64, against torch.optim.Adam after clamp_."""
    case = ("f64", 257)
    s = DC.adam_inputs(case)
    w = s["p"].clone().requires_grad_()
    opt = torch.optim.Adam([w], lr=DC.ADAM["lr"], betas=(DC.ADAM["beta1"], DC.ADAM["beta2"]), eps=DC.ADAM["eps"])
    p, m, v = s["p"], s["m"], s["v"]
    opt.state[w] = dict(step=torch.tensor(0.0), exp_avg=m.clone(), exp_avg_sq=v.clone())  # non-zero moments
    for step in range(1, DC.ADAM_STEPS + 1):
        g = s["g"][step - 1]
        w.grad = g.clone().clamp_(-DC.ADAM["clip"], DC.ADAM["clip"])
        opt.step()
        r = DC.adam_ref(p, g, m, v, step, F64)
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        st = opt.state[w]
        errs = rel_err(p, w), rel_err(m, st["exp_avg"]), rel_err(v, st["exp_avg_sq"])
        print(f"adam reference vs torch.optim.Adam step {step}:", errs)
        assert max(errs) <= 1e-12, errs


# ------------------------------------------------------------------------------------------ b. headroom
def run(name, case, dt=F64, bug=None):
    """(inputs, reference outputs) of one case of kernel family ``name``"""
    p = getattr(DC, f"{name}_inputs")(case)
    ref = getattr(DC, f"{name}_ref")
    bt = {"softctx": 3, "fwdf": 6, "scoreb": 3, "bwdf": 6, "lstm_bwd": 2}.get(name)
    args = (p,) if bt is None else (p, case[bt])
    kw = dict(dt=dt) if bug is None else dict(dt=dt, bug=bug)
    return p, ref(*args, **kw)


def compare(name, case, got, ref, p, what):
    if name == "score":
        got = {k: v for k, v in got.items() if k == "e" or case[6]}
        DC.score_compare(got, ref, case[3], what)
    elif name == "softctx":
        DC.softctx_compare(got, ref, case[3], what)
    elif name == "fwdf":
        DC.fwdf_compare(got, ref, p, case[6], what)
    elif name == "scoreb":
        DC.scoreb_compare(got, ref, case[3], what)
    elif name == "bwdf":
        DC.bwdf_compare(got, ref, case[6], what)
    elif name == "lstm_bwd":
        DC.lstm_bwd_compare(got, ref, case[2], what)
    else:
        getattr(DC, f"{name}_compare")(got, ref, what)


FAMILIES = [("mean", DC.MEAN_CASES), ("score", DC.SCORE_CASES), ("softctx", DC.SOFTCTX_CASES), ("fwdf", DC.FWDF_CASES),
            ("ctxb", DC.CTXB_CASES), ("scoreb", DC.SCOREB_CASES), ("bwdf", DC.BWDF_CASES), ("dinput", DC.DINPUT_CASES),
            ("encgrad", DC.ENCGRAD_CASES), ("lstm_fwd", DC.LSTM_FWD_CASES), ("lstm_bwd", DC.LSTM_BWD_CASES), ("ce", DC.CE_CASES),
            ("reg", DC.REG_CASES)]


@pytest.mark.parametrize("name,case", [(n, c) for n, cs in FAMILIES for c in cs],
                         ids=lambda v: v if isinstance(v, str) else DC.case_id(v))
def test_fp32_emulation_passes(name, case):
    """The reference recomputed in fp32 on the CPU passes the comparison the GPU test makes, with room to spare."""
    p, ref = run(name, case)
    _, lo = run(name, case, F32)
    before = dict(DC.RATIOS)
    compare(name, case, emu(lo), ref, p, f"emulated {name} {DC.case_id(case)}")
    new = {k: v for k, v in DC.RATIOS.items() if k.startswith(f"emulated {name} ") and before.get(k) != v}
    # (a ``roundings`` count can be reached: up to 1, which ``compare`` has asserted)
    worst = max([v for k, v in new.items() if not k.endswith(("att_dec_out", "ad_out", "dlogits", "dreg"))] + [0.0])
    assert worst <= 0.5, new


def adam_emulate(p, g, m, v, step, T):
    """csrc/optim.hip's arithmetic in T, one rounding per operation"""
    h = DC.ADAM
    c = lambda x: torch.tensor(x, dtype=F64).to(T)  # noqa: E731
    bc1, bc2s = DC.adam_bc(step)
    step_size, bc2 = c(h["lr"] / bc1), c(bc2s)
    gi = g.clamp(-h["clip"], h["clip"])
    mi = m + c(1 - h["beta1"]) * (gi - m)
    vi = v * c(h["beta2"]) + (c(1 - h["beta2"]) * gi) * gi
    return dict(m=mi, v=vi, p=p + (-step_size) * (mi / (vi.sqrt() / bc2 + c(h["eps"]))))


@pytest.mark.parametrize("case", [c for c in DC.ADAM_CASES if c[1] <= 257], ids=DC.case_id)
def test_adam_emulation_passes(case):
    T = DC.adam_dtype(case)
    s = DC.adam_inputs(case)
    st = {k: s[k] for k in "pmv"}
    for step in range(1, DC.ADAM_STEPS + 1):
        g = s["g"][step - 1]
        ref = DC.adam_ref(st["p"], g, st["m"], st["v"], step, T)
        st = adam_emulate(st["p"], g, st["m"], st["v"], step, T)
        assert st["p"].dtype == T
        DC.adam_compare(st, ref, T, f"emulated adam {DC.case_id(case)}")
    special = s["g"][0][:6].abs()
    assert case[1] < 6 or (float(special[0]) == DC.ADAM["clip"] and float(special[2]) < DC.ADAM["clip"] < float(special[4]))


@pytest.mark.parametrize("case", DC.SCATTER_CASES, ids=DC.case_id)
def test_scatter_emulation_passes(case):
    p = DC.scatter_inputs(case)
    ref = DC.scatter_ref(p)
    T = p["demb"].dtype
    got = DC.scatter_ref(p, dt=T)[0]
    DC.scatter_compare(got, ref, p["demb"], f"emulated scatter {DC.case_id(case)}")
    mult = sorted(set(ref[2].tolist()))
    want = {("mixed", 1): [0, 1, 2, 6], ("same", 0): [0, 12], ("same", 1): [0, 9]}[case[1:]]
    assert mult == want, mult


def test_loss_finalize_and_movers_references():
    for case in DC.LOSSFIN_CASES:
        p = DC.lossfin_inputs(case)
        DC.within(DC.lossfin_ref(p, F32)["loss"][0], *DC.lossfin_ref(p)["loss"], f"emulated loss_finalize {case}")
    p = DC.gather_inputs(("f64", 300))
    out = DC.gather_ref(p)
    assert out.shape == (DC.EMB_T, DC.EMB_B, 300) and out.dtype == F32
    assert bool((out[2, 1] == p["emb"][p["caps"][1, 2]].float()).all())
    x = torch.ones(DC.MASK_T, DC.MASK_B, DC.MASK_COLS)
    assert DC.mask_ref(x).sum() == DC.MASK_COLS * sum(DC.MASK_BT)


def test_inputs_stay_in_range():
    """Pre-activations and logits within [-4, 4], scores within [-2, 2]: exp arguments cost a few ulp at most."""
    for c in DC.SOFTCTX_CASES:
        p = DC.softctx_inputs(c)
        assert float(p["e"].abs().max()) <= 2
        if p["gate_parts"] is not None:
            assert float(DC.slab_total(p["gate_parts"], p["bias_fb"])[0].abs().max()) <= 4
    for name, cases in (("score", DC.SCORE_CASES), ("fwdf", DC.FWDF_CASES)):
        for c in cases:
            p, ref = run(name, c)
            e = ref["e"][0] if name == "score" else DC.scores(p["att_enc"], ref["ad"][0], ref["ad"][1], p["wf"], p["bf"], F64)[0]
            assert float(e.abs().max()) <= 2 + 1e-6, (name, c)
    for c in DC.LSTM_FWD_CASES:
        p = DC.lstm_fwd_inputs(c)
        first = DC.slab_total(p["parts"], p["xemb"])[0] if (c[2] or c[4]) else None
        assert float(DC.slab_total(p["hh_parts"], first)[0].abs().max()) <= 4
    for c in DC.CE_CASES:
        p = DC.ce_inputs(c)
        assert float(p["logits"].abs().max()) <= 4
        tg = p["caps"][:, 1:DC.CE_T + 1]
        assert int(tg.min()) == 0 and int(tg.max()) == c[0] - 1


# ------------------------------------------------------------------------------------------ c. teeth
def bugged(name, case, bug):
    p, ref = run(name, case)
    _, bad = run(name, case, F32, bug)
    return p, ref, emu(bad)


def test_dropped_last_slab_of_13_fails():
    case = DC.SCORE_CASES[4]
    assert case[3] == 13
    p, ref, got = bugged("score", case, "drop_last_slab")
    fails(DC.roundings, got["att_dec"], *ref["att_dec"], 13, "att_dec without the last slab")
    fails(DC.within, got["e"], *ref["e"], "e without the last slab")
    case = DC.SOFTCTX_CASES[2]
    assert case[4] == 13
    p, ref, got = bugged("softctx", case, "drop_last_slab")
    fails(DC.within, got["gate"], *ref["gate"], "gate without the last slab")
    fails(DC.within, got["x"], *ref["x"], "x without the last slab")
    case = DC.LSTM_FWD_CASES[2]
    p, ref, got = bugged("lstm_fwd", case, "drop_last_slab")
    for k in ("act", "c", "h"):
        fails(DC.within, got[k], *ref[k], f"lstm {k} without the last slab")
    p, ref, got = bugged("ctxb", DC.CTXB_CASES[3], "drop_last_slab")
    for k in ("dawe", "dgp", "dalpha"):
        fails(DC.within, got[k], *ref[k], f"att_ctx_bwd {k} without the last slab")
    p, ref, got = bugged("fwdf", DC.FWDF_CASES[1], "drop_last_slab")
    fails(DC.roundings, got["ad"], *ref["ad"], 3, "fused ad_out without the last slab")
    fails(DC.within, got["alpha"], *ref["alpha"], "fused alpha without the last slab")


def test_dropped_tail_rows_of_29_fail():
    p, ref, got = bugged("score", DC.SCORE_CASES[3], "drop_tail_rows")
    assert float(got["e"][:, 26:].abs().max()) == 0 and float(got["e"][:, :26].abs().min()) > 0
    fails(DC.within, got["e"], *ref["e"], "e without rows 26..28")
    p, ref, got = bugged("ctxb", DC.CTXB_CASES[3], "drop_tail_rows")
    fails(DC.within, got["dalpha"], *ref["dalpha"], "dalpha without rows 26..28")
    p, ref, got = bugged("scoreb", DC.SCOREB_CASES[4], "drop_tail_rows")
    fails(DC.within, got["dad"], *ref["dad"], "dad without rows 26..28")
    p, ref, got = bugged("encgrad", DC.ENCGRAD_CASES[2], "drop_tail_rows")
    fails(DC.within, got["wf_grad"], *ref["wf_grad"], "wf_grad without rows 26..28")
    fails(DC.within, got["bf_grad"], *ref["bf_grad"], "bf_grad without rows 26..28")


def test_skipped_p_group_fails():
    for name, case in (("softctx", DC.SOFTCTX_CASES[1]), ("softctx", DC.SOFTCTX_CASES[2]), ("fwdf", DC.FWDF_CASES[3])):
        p, ref, got = bugged(name, case, "skip_pgroup3")
        fails(DC.within, got["awe"], *ref["awe"], f"{name} awe without p-group 3")
        fails(DC.within, got["x"], *ref["x"], f"{name} x without p-group 3")


def test_alpha_stride_taken_as_P_fails():
    case = DC.SCOREB_CASES[4]
    p, ref, got = bugged("scoreb", case, "alpha_ld_is_P")
    fails(DC.within, got["de"], *ref["de"], "de with alpha_ld_b = P")
    fails(DC.scoreb_compare, got, ref, case[3], "att_score_bwd with alpha_ld_b = P")


def test_rows_past_bt_not_zeroed_fail():
    for name, case, bt in (("softctx", DC.SOFTCTX_CASES[1], 2), ("fwdf", DC.FWDF_CASES[1], 2), ("scoreb", DC.SCOREB_CASES[1], 1),
                           ("bwdf", DC.BWDF_CASES[1], 1), ("lstm_bwd", DC.LSTM_BWD_CASES[1], 1)):
        p, ref, got = bugged(name, case, "bt_ignored")
        fails(compare, name, case, got, ref, p, f"{name} with bt ignored")
        key = {"softctx": "alpha", "fwdf": "alpha", "scoreb": "de", "bwdf": "de", "lstm_bwd": "dc_out"}[name]
        fails(DC.all_zero, got[key][bt:], f"{name} {key} rows b >= bt")


def test_swapped_f_and_g_gates_fail():
    p, ref, got = bugged("lstm_fwd", DC.LSTM_FWD_CASES[1], "swap_f_g")
    for k in ("act", "c", "h"):
        fails(DC.within, got[k], *ref[k], f"lstm forward {k} with f and g swapped")
    p, ref, got = bugged("lstm_bwd", DC.LSTM_BWD_CASES[3], "swap_f_g")
    fails(DC.within, got["dgates"], *ref["dgates"], "lstm backward dgates with f and g swapped")
    fails(DC.within, got["dc_out"], *ref["dc_out"], "lstm backward dc_out with f and g swapped")


def test_ce_bugs_fail():
    case = DC.CE_CASES[1]
    p, ref, got = bugged("ce", case, "target_at_t")
    fails(DC.within, got["loss"], *ref["loss"], "loss with the target read at t")
    fails(DC.roundings, got["dlogits"], *ref["dlogits"], ref["k"], "dlogits with the target read at t")
    assert case[2] == 1
    p, ref, got = bugged("ce", case, "batch_major")
    fails(DC.roundings, got["dlogits"], *ref["dlogits"], ref["k"], "dlogits batch-major for time-major")
    DC.within(got["loss"], *ref["loss"], "loss (unaffected)")


def test_reg_and_dmean_scale_bugs_fail():
    p, ref, got = bugged("reg", DC.REG_CASES[1], "scaled_by_1_over_P")
    fails(DC.roundings, got["dreg"], *ref["dreg"], ref["k"], "dreg scaled by 1 / P")
    p, ref, got = bugged("dinput", DC.DINPUT_CASES[1], "dmean_not_divided")
    fails(DC.within, got["denc"], *ref["denc"], "denc with dmean not divided by P")


@pytest.mark.parametrize("case", [("f32", 257), ("f64", 257)], ids=DC.case_id)
def test_adam_bugs_fail(case):
    T = DC.adam_dtype(case)
    s = DC.adam_inputs(case)
    ulp = DC.ULP if T == F32 else 2.0 ** -53
    for bug, outs in (("bias_correction_of_t_minus_1", "p"), ("no_clamp", "mvp")):
        good = DC.adam_ref(s["p"], s["g"][1], s["m"], s["v"], 2, T)
        bad = DC.adam_ref(s["p"], s["g"][1], s["m"], s["v"], 2, T, bug)
        for k in outs:
            fails(DC.roundings, bad[k][0].to(T), *good[k], DC.ADAM_K[k], f"adam {k} with {bug}", ulp)


def test_overwriting_scatter_fails():
    for case in DC.SCATTER_CASES:
        p = DC.scatter_inputs(case)
        ref = DC.scatter_ref(p)
        bad = DC.scatter_ref(p, dt=p["demb"].dtype, bug="overwrite")[0]
        fails(DC.scatter_compare, bad, ref, p["demb"], f"overwriting scatter {DC.case_id(case)}")


def test_roundings_has_no_floor():
    """an error of 1e-9 on a value of 1e-7 passes ``within`` and fails ``roundings``"""
    ref, mag = torch.full((4,), 1e-7, dtype=F64), torch.full((4,), 1e-7, dtype=F64)
    got = (ref + 1e-9).float()
    DC.within(got, ref, mag, "floor")
    fails(DC.roundings, got, ref, mag, 16, "no floor")
    assert DC.roundings((ref * (1 + 8 * DC.ULP)).float(), ref, mag, 16, "k ulp") <= 1
    assert math.isclose(DC.ULP, 2.0 ** -24)
