"""GPU: the kernels behind the baseline captioner's training step (csrc/baseline_step.hip, csrc/loss.hip).

capmi_lstm_step_fwd_train: h / c are capmi_lstm_step_fwd's bits, act_out against the fp64 formula. capmi_lstm_step_bwd
against the fp64 formula. Neither tolerance is a constant: in the same test the sequence the fused launch stands for
(capmi_gemm TILE_64 with capmi_lstm_cell_fwd / capmi_lstm_cell_bwd) runs on the same inputs, and the fused kernel's
relative L2 error may be at most twice that sequence's. capmi_count_targets / capmi_ce_ignore_fwd_bwd /
capmi_loss_finalize_dev against fp64 F.cross_entropy(ignore_index=0) with ce_compare's rounding budget."""
import math

import pytest
import torch

import decoder_kernel_cases as DC
import gen
from helpers import rel_err, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = 1001
CANARY = 777.0


def _close(got, want):
    """The project's loss tolerance (tests/test_gpu_eval.py)."""
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


def _canaried(R, cols):
    return torch.full((R + 2, cols), CANARY, device=DEV)


def _take(buf, R):
    """The R written rows; the two canary rows after them must be untouched."""
    assert (buf[R:] == CANARY).all()
    return buf[:R].cpu()


# ---------------------------------------------------------------------------------------------------
# capmi_lstm_step_fwd_train
# ---------------------------------------------------------------------------------------------------
def _fwd_inputs(R, M, H, seed=3):
    b = 1.0 / math.sqrt(H)
    u = lambda name, shape, lo=-1.0, hi=1.0: t(gen.uniform(seed, name, shape, lo, hi))  # noqa: E731
    return dict(h=u("h", (R, H)), c=u("c", (R, H)), pre=u("pre", (R, 4 * H)), w_hh=u("w_hh", (4 * H, H), -b, b))


def _act64(d, first):
    g = d["pre"].double()
    if not first:
        g = g + d["h"].double() @ d["w_hh"].double().T
    i, f, gg, o = g.chunk(4, 1)
    return torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], 1)


FWD_SHAPES = [(R, M, H) for R in (1, 3, 65) for H in (16, 24, 512) for M in (16, 20, 512)] + [(64, 512, 512)]


@pytest.mark.parametrize("R,M,H", FWD_SHAPES)
def test_fwd_train_is_the_inference_step_plus_activations(R, M, H):
    """M sizes nothing here (the training step takes x W_ih^T hoisted, as ``pre``); it is passed through."""
    from capmi import kernels as K
    from capmi._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_NMAJOR_W as BW
    d = _fwd_inputs(R, M, H)
    g = {k: v.to(DEV) for k, v in d.items()}
    f = dict(device=DEV, dtype=torch.float32)
    for first in (False, True):
        kw = dict(pre=g["pre"]) if first else dict(pre=g["pre"], h_prev=g["h"], c_prev=g["c"], w_hh=g["w_hh"])
        h, c, act = _canaried(R, H), _canaried(R, H), _canaried(R, 4 * H)
        K.lstm_step_fwd_train(R, M, H, h, c, act, **kw)
        h0, c0 = _canaried(R, H), _canaried(R, H)
        K.lstm_step_fwd(R, M, H, h0, c0, **kw)
        # the sequence it stands for: capmi_gemm TILE_64, capmi_lstm_cell_fwd
        hh = None
        if not first:
            hh = torch.empty(R, 4 * H, **f)
            K.gemm(K.problem(R, 4 * H, H, g["h"], H, g["w_hh"], H, hh, 4 * H), AK, BW, K.TILE_64)
        eh, ec, eact = torch.empty(R, H, **f), torch.empty(R, H, **f), torch.empty(R, 4 * H, **f)
        K.lstm_cell_fwd(g["pre"], 1, 0, None, hh, 0 if first else 1, 0, torch.zeros(R, H, **f) if first else g["c"],
                        R, H, eh, ec, eact)
        torch.cuda.synchronize()
        assert torch.equal(_take(h, R), _take(h0, R)) and torch.equal(_take(c, R), _take(c0, R))
        want = _act64(d, first)
        e_new, e_old = rel_err(_take(act, R), want), rel_err(eact, want)
        print(f"R={R} M={M} H={H} first={first}: act fused {e_new:.3g}; existing {e_old:.3g}")
        assert e_new <= 2 * e_old, (first, e_new, e_old)


def test_fwd_train_rejects_bad_arguments_without_launching():
    from capmi import kernels as K
    from capmi._lib import CapmiError
    R, M, H = 2, 16, 8
    g = {k: v.to(DEV) for k, v in _fwd_inputs(R, M, H).items()}
    h, c, act = (torch.full((R, n), 9.0, device=DEV) for n in (H, H, 4 * H))
    kw = dict(pre=g["pre"], h_prev=g["h"], c_prev=g["c"], w_hh=g["w_hh"])
    with pytest.raises(CapmiError, match=str(EINVAL)):  # no act_out
        K.lstm_step_fwd_train(R, M, H, h, c, None, **kw)
    with pytest.raises(CapmiError, match=str(EINVAL)):  # act_out is an input
        K.lstm_step_fwd_train(R, M, H, h, c, g["pre"], **kw)
    torch.cuda.synchronize()
    assert (h == 9.0).all() and (c == 9.0).all() and (act == 9.0).all()


# ---------------------------------------------------------------------------------------------------
# capmi_lstm_step_bwd
# ---------------------------------------------------------------------------------------------------
def _bwd_inputs(R, H, seed=6):
    b = 1.0 / math.sqrt(H)
    u = lambda name, shape, lo=-1.0, hi=1.0: t(gen.uniform(seed, name, shape, lo, hi))  # noqa: E731
    i, f, gg, o = u("gates", (R, 4 * H), -2.0, 2.0).double().chunk(4, 1)
    act = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], 1).float()
    return dict(act=act, c_prev=u("c_prev", (R, H)), c_cur=u("c_cur", (R, H)), dh_lin=u("dh_lin", (R, H)),
                dc_in=u("dc_in", (R, H)), dg_next=u("dg_next", (R, 4 * H), -0.5, 0.5),
                w_hh=u("w_hh", (4 * H, H), -b, b))


BWD_FORMS = {
    "last": ("dh_lin",),                     # no dg_next, no dc_in: no GEMM
    "middle": ("dh_lin", "dg_next", "dc_in"),
    "no_dh_lin": ("dg_next", "dc_in"),
}


def _bwd64(d, use):
    x = {k: v.double() for k, v in d.items()}
    R, H = d["c_cur"].shape
    dh = torch.zeros(R, H, dtype=torch.float64)
    if "dh_lin" in use:
        dh = dh + x["dh_lin"]
    if "dg_next" in use:
        dh = dh + x["dg_next"] @ x["w_hh"]
    ig, fg, cg, og = x["act"].chunk(4, 1)
    tc = torch.tanh(x["c_cur"])
    d_o = dh * tc * og * (1 - og)
    dc = (x["dc_in"] if "dc_in" in use else 0) + dh * og * (1 - tc * tc)
    dg = torch.cat([dc * cg * ig * (1 - ig), dc * x["c_prev"] * fg * (1 - fg), dc * ig * (1 - cg * cg), d_o], 1)
    return dg, dc * fg


def _bwd_fused(g, use, R, H):
    from capmi import kernels as K
    dg, dc = _canaried(R, 4 * H), _canaried(R, H)
    K.lstm_step_bwd(R, H, g["act"], g["c_cur"], dg, dc, dh_lin=g["dh_lin"] if "dh_lin" in use else None,
                    dg_next=g["dg_next"] if "dg_next" in use else None, w_hh=g["w_hh"],
                    dc_in=g["dc_in"] if "dc_in" in use else None, c_prev=g["c_prev"])
    torch.cuda.synchronize()
    return _take(dg, R), _take(dc, R)


def _bwd_existing(g, use, R, H):
    """capmi_gemm TILE_64 (B_KROWS) into capmi_lstm_cell_bwd: the autograd path's step."""
    from capmi import kernels as K
    from capmi._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_KROWS as BKR
    f = dict(device=DEV, dtype=torch.float32)
    dhr = None
    if "dg_next" in use:
        dhr = torch.empty(R, H, **f)
        K.gemm(K.problem(R, H, 4 * H, g["dg_next"], 4 * H, g["w_hh"], H, dhr, H), AK, BKR, K.TILE_64)
    dg, dc = torch.empty(R, 4 * H, **f), torch.empty(R, H, **f)
    K.lstm_cell_bwd(g["dh_lin"] if "dh_lin" in use else None, dhr, 1 if dhr is not None else 0, 0,
                    g["dc_in"] if "dc_in" in use else None, g["act"], g["c_prev"], g["c_cur"], R, H, R, dg, dc)
    torch.cuda.synchronize()
    return dg.cpu(), dc.cpu()


BWD_SHAPES = [(R, H) for R in (1, 3, 65) for H in (16, 24, 512)] + [(64, 512)]


@pytest.mark.parametrize("R,H", BWD_SHAPES)
def test_bwd_step_matches_fp64_within_twice_the_existing_path(R, H):
    d = _bwd_inputs(R, H)
    g = {k: v.to(DEV) for k, v in d.items()}
    for name, use in BWD_FORMS.items():
        want_dg, want_dc = _bwd64(d, use)
        dg, dc = _bwd_fused(g, use, R, H)
        edg, edc = _bwd_existing(g, use, R, H)
        errs = (rel_err(dg, want_dg), rel_err(dc, want_dc), rel_err(edg, want_dg), rel_err(edc, want_dc))
        print(f"R={R} H={H} {name}: fused dgates {errs[0]:.3g} dc {errs[1]:.3g}; "
              f"existing dgates {errs[2]:.3g} dc {errs[3]:.3g}")
        assert errs[0] <= 2 * errs[2], (name, errs)
        assert errs[1] <= 2 * errs[3], (name, errs)


@pytest.mark.parametrize("H", [24, 512])
def test_bwd_step_rows_do_not_depend_on_the_batch_and_runs_are_identical(H):
    R = 65
    g = {k: v.to(DEV) for k, v in _bwd_inputs(R, H, seed=7).items()}
    use = BWD_FORMS["middle"]
    dg, dc = _bwd_fused(g, use, R, H)
    dg2, dc2 = _bwd_fused(g, use, R, H)
    assert torch.equal(dg, dg2) and torch.equal(dc, dc2)  # two runs: the same bits
    for r in (0, 17, 63, 64):
        one = {k: (v if k == "w_hh" else v[r:r + 1].contiguous()) for k, v in g.items()}
        dg1, dc1 = _bwd_fused(one, use, 1, H)
        assert torch.equal(dg1[0], dg[r]) and torch.equal(dc1[0], dc[r]), r


def test_bwd_step_rejects_bad_arguments_without_launching():
    from capmi import kernels as K
    from capmi._lib import CapmiError
    R, H = 2, 8
    g = {k: v.to(DEV) for k, v in _bwd_inputs(R, H).items()}
    dg, dc = torch.full((R, 4 * H), 9.0, device=DEV), torch.full((R, H), 9.0, device=DEV)
    kw = dict(dh_lin=g["dh_lin"], dg_next=g["dg_next"], w_hh=g["w_hh"], dc_in=g["dc_in"], c_prev=g["c_prev"])
    with pytest.raises(CapmiError, match=str(EINVAL)):  # H % 4 != 0
        K.lstm_step_bwd(R, 6, g["act"], g["c_cur"], dg, dc, dh_lin=g["dh_lin"], dc_in=g["dc_in"], c_prev=g["c_prev"])
    with pytest.raises(CapmiError, match=str(EINVAL)):  # dgates is dg_next
        K.lstm_step_bwd(R, H, g["act"], g["c_cur"], g["dg_next"], dc, **kw)
    with pytest.raises(CapmiError, match=str(EINVAL)):  # dc_out is dc_in
        K.lstm_step_bwd(R, H, g["act"], g["c_cur"], dg, g["dc_in"], **kw)
    with pytest.raises(CapmiError, match=str(EINVAL)):  # no act
        K.lstm_step_bwd(R, H, None, g["c_cur"], dg, dc, **kw)
    with pytest.raises(CapmiError, match=str(EINVAL)):  # dg_next without W_hh
        K.lstm_step_bwd(R, H, g["act"], g["c_cur"], dg, dc, **dict(kw, w_hh=None))
    torch.cuda.synchronize()
    assert (dg == 9.0).all() and (dc == 9.0).all()


# ---------------------------------------------------------------------------------------------------
# capmi_count_targets, capmi_ce_ignore_fwd_bwd, capmi_loss_finalize_dev
# ---------------------------------------------------------------------------------------------------
CE_B, CE_T = 3, 4


def _ce_inputs(V, tgt_off):
    """Targets 0 (ignored) and V - 1 both occur, caption 2 is ignored entirely, the rest is live."""
    L = CE_T + (3 if tgt_off else 0)
    g = DC.gen("ce_ignore", (V, tgt_off))
    caps = torch.randint(1, V, (CE_B, L), generator=g)
    caps[0, tgt_off + 1] = 0
    caps[1, tgt_off + 2] = V - 1
    caps[1, tgt_off + 3] = 0
    caps[2, tgt_off:tgt_off + CE_T] = 0
    return DC._u(g, (CE_B, CE_T, V), 4.0), caps, L


@pytest.mark.parametrize("tm", [0, 1])
@pytest.mark.parametrize("tgt_off", [0, 2])
@pytest.mark.parametrize("V", [7, 257, 8100])
def test_ce_ignore_index_matches_fp64_cross_entropy(V, tgt_off, tm):
    from capmi import kernels as K
    import torch.nn.functional as F
    B, T = CE_B, CE_T
    x, caps, L = _ce_inputs(V, tgt_off)
    tgt = caps[:, tgt_off:tgt_off + T]
    live = tgt != 0
    n = int(live.sum())
    assert 0 < n < B * T and not live[2].any() and (tgt == V - 1).any()
    xd, cd = x.to(DEV), caps.to(DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    inv = torch.full((1,), -1.0, device=DEV)
    rows, dl, loss = _canaried(B * T, 1), _canaried(B * T, V), torch.full((1,), -1.0, device=DEV)
    K.count_targets(cd, B, T, L, tgt_off, 0, count, inv)
    K.ce_ignore_fwd_bwd(xd, cd, B, T, L, V, tgt_off, 0, inv, rows, dl, bool(tm))
    K.loss_finalize_dev(rows, B * T, inv, loss)
    torch.cuda.synchronize()
    assert int(count) == n and abs(float(inv) - 1.0 / n) <= 2.0 ** -23 / n
    want = float(F.cross_entropy(x.double().reshape(B * T, V), tgt.reshape(-1), ignore_index=0))
    print(f"V={V} tgt_off={tgt_off} tm={tm}: loss {float(loss):.8g} want {want:.8g}")
    assert _close(float(loss), want), (float(loss), want)
    # rows and gradient: capmi_ce_fwd_bwd's per-row arithmetic, so its reference and budget (ce_compare) with
    # the targets moved to column t + 1 and g = 1 / n
    ref = DC.ce_ref(dict(logits=x, caps=torch.cat([tgt[:, :1], tgt], 1), bt=None, gscale=None, nrows=n, tm=tm))
    lv = live[..., None]
    dl_ref = ref["dlogits"][0].view(*((T, B) if tm else (B, T)), V)
    dl_ref = dl_ref * (lv.transpose(0, 1) if tm else lv)
    ref["live"] = live
    ref["loss"] = (ref["loss"][0] * live, ref["loss"][1])
    ref["dlogits"] = (dl_ref.reshape(B * T, V), ref["dlogits"][1])
    DC.ce_compare(dict(loss=_take(rows, B * T).view(B, T), dlogits=_take(dl, B * T)), ref, f"ce_ignore V={V}")
    got_dl = dl[:B * T].cpu().view(*((T, B) if tm else (B, T)), V)
    dead = (~live).transpose(0, 1) if tm else ~live
    DC.all_zero(got_dl[dead], "dlogits of ignored rows")
    DC.all_zero(rows[:B * T].cpu().view(B, T)[~live], "loss_rows of ignored rows")


def test_ce_without_a_live_target_is_nan_as_torch():
    from capmi import kernels as K
    B, T, V = 2, 3, 7
    x = DC._u(DC.gen("ce_ignore_nan", (V,)), (B, T, V), 4.0).to(DEV)
    caps = torch.zeros(B, T, dtype=torch.int64, device=DEV)
    count, inv = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)
    rows, loss = torch.ones(B * T, device=DEV), torch.zeros(1, device=DEV)
    K.count_targets(caps, B, T, T, 0, 0, count, inv)
    K.ce_ignore_fwd_bwd(x, caps, B, T, T, V, 0, 0, inv, rows)
    K.loss_finalize_dev(rows, B * T, inv, loss)
    torch.cuda.synchronize()
    assert int(count) == 0 and math.isnan(float(loss))
