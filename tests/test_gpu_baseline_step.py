"""GPU: the kernels behind the baseline captioner's inference (csrc/baseline_step.hip, csrc/eval.hip).

capmi_lstm_step_fwd against the fp64 formula. Its tolerance is not a constant: in the same test the existing
three-launch sequence (capmi_gemm TILE_64 for the products, then capmi_lstm_cell_fwd) runs on the same inputs,
and the fused kernel's relative L2 error on h and on c may be at most twice that sequence's (a different but
equally long fp32 summation order). capmi_eval_rows_at / capmi_eval_captions_ce against the fp64 restatements
of tests/eval_cases.py and tests/baseline_cases.py."""
import math

import numpy as np
import pytest
import torch

import baseline_cases as BC
import eval_cases as EC
import gen
from helpers import rel_err, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
EINVAL = 1001


def _close(got, want):
    """The project's loss tolerance (tests/test_gpu_eval.py)."""
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


# ---------------------------------------------------------------------------------------------------
# capmi_lstm_step_fwd
# ---------------------------------------------------------------------------------------------------
def _inputs(R, M, H, seed=3):
    b = 1.0 / math.sqrt(H)
    u = lambda name, shape, lo=-1.0, hi=1.0: t(gen.uniform(seed, name, shape, lo, hi))  # noqa: E731
    return dict(x=u("x", (R, M)), h=u("h", (R, H)), c=u("c", (R, H)), pre=u("pre", (R, 4 * H)),
                w_ih=u("w_ih", (4 * H, M), -b, b), w_hh=u("w_hh", (4 * H, H), -b, b),
                b_ih=u("b_ih", (4 * H,), -b, b), b_hh=u("b_hh", (4 * H,), -b, b))


def _ref64(d, use):
    """The formula in fp64 on the terms named in ``use``."""
    R, H = d["h"].shape
    g = torch.zeros(R, 4 * H, dtype=torch.float64)
    if "pre" in use:
        g = g + d["pre"].double()
    if "x" in use:
        g = g + d["x"].double() @ d["w_ih"].double().T
    if "h" in use:
        g = g + d["h"].double() @ d["w_hh"].double().T
    if "bias" in use:
        g = g + d["b_ih"].double() + d["b_hh"].double()
    i, f, gg, o = g.chunk(4, 1)
    c = torch.sigmoid(i) * torch.tanh(gg)
    if "c" in use:
        c = c + torch.sigmoid(f) * d["c"].double()
    return torch.sigmoid(o) * torch.tanh(c), c


def _dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _fused(g, use, R, M, H, ld_pre=0, ld_x=0, canary=True):
    """h, c (R, H) of the fused kernel; two canary rows after each output must stay untouched."""
    from capmi import kernels as K
    h_out = torch.full((R + 2, H), 777.0, device=DEV)
    c_out = torch.full((R + 2, H), 777.0, device=DEV)
    pre, x = g["pre"], g["x"]
    if ld_pre:
        wide = torch.full((R, ld_pre), 55.0, device=DEV)
        wide[:, :4 * H] = pre
        pre = wide
    if ld_x:
        wide = torch.full((R, ld_x), 55.0, device=DEV)
        wide[:, :M] = x
        x = wide
    K.lstm_step_fwd(R, M, H, h_out, c_out, pre=pre if "pre" in use else None, ld_pre=ld_pre,
                    x=x if "x" in use else None, ld_x=ld_x, h_prev=g["h"] if "h" in use else None,
                    c_prev=g["c"] if "c" in use else None, w_ih=g["w_ih"] if "x" in use else None,
                    w_hh=g["w_hh"] if "h" in use else None, b_ih=g["b_ih"] if "bias" in use else None,
                    b_hh=g["b_hh"] if "bias" in use else None)
    torch.cuda.synchronize()
    assert (h_out[R:] == 777.0).all() and (c_out[R:] == 777.0).all()
    return h_out[:R].cpu(), c_out[:R].cpu()


def _existing(g, use, R, M, H):
    """The training forward's sequence: capmi_gemm TILE_64 per product, then capmi_lstm_cell_fwd."""
    from capmi import kernels as K
    from capmi._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_NMAJOR_W as BW
    f = dict(device=DEV, dtype=torch.float32)
    part = g["pre"] if "pre" in use else None
    if "x" in use:
        gx = torch.empty(R, 4 * H, **f)
        bias = dict(bias=g["b_ih"], bias2=g["b_hh"]) if "bias" in use else {}
        K.gemm(K.problem(R, 4 * H, M, g["x"], M, g["w_ih"], M, gx, 4 * H, **bias), AK, BW, K.TILE_64)
        assert part is None
        part = gx
    hh = None
    if "h" in use:
        hh = torch.empty(R, 4 * H, **f)
        K.gemm(K.problem(R, 4 * H, H, g["h"], H, g["w_hh"], H, hh, 4 * H), AK, BW, K.TILE_64)
    c_prev = g["c"] if "c" in use else torch.zeros(R, H, **f)
    h_out, c_out, act = torch.empty(R, H, **f), torch.empty(R, H, **f), torch.empty(R, 4 * H, **f)
    K.lstm_cell_fwd(part, 1, 0, None, hh, 1 if hh is not None else 0, 0, c_prev, R, H, h_out, c_out, act)
    torch.cuda.synchronize()
    return h_out.cpu(), c_out.cpu()


FORMS = {
    "pre+h": ("pre", "h", "c"),            # the validation pass: x = NULL, NULL biases
    "x+h+bias": ("x", "h", "c", "bias"),   # the beam search step
    "first": ("x", "bias"),                # the first step: h_prev = c_prev = NULL
}
SHAPES = [(R, M, H) for R in (1, 3, 65) for H in (16, 24, 512) for M in (16, 20, 512)] + [(320, 512, 512)]


@pytest.mark.parametrize("R,M,H", SHAPES)
def test_lstm_step_matches_fp64_within_twice_the_existing_path(R, M, H):
    d = _inputs(R, M, H)
    g = _dev(d)
    for name, use in FORMS.items():
        want_h, want_c = _ref64(d, use)
        h, c = _fused(g, use, R, M, H)
        eh, ec = _existing(g, use, R, M, H)
        errs = (rel_err(h, want_h), rel_err(c, want_c), rel_err(eh, want_h), rel_err(ec, want_c))
        print(f"R={R} M={M} H={H} {name}: fused h {errs[0]:.3g} c {errs[1]:.3g}; existing h {errs[2]:.3g} c {errs[3]:.3g}")
        assert errs[0] <= 2 * errs[2], (name, errs)
        assert errs[1] <= 2 * errs[3], (name, errs)


@pytest.mark.parametrize("R,M,H", [(3, 20, 24), (65, 512, 512)])
def test_lstm_step_leading_dimensions(R, M, H):
    """pre / x as slices of wider rows give the bits of the dense call."""
    d = _inputs(R, M, H, seed=4)
    g = _dev(d)
    for use in (FORMS["pre+h"], FORMS["x+h+bias"]):
        h, c = _fused(g, use, R, M, H)
        h2, c2 = _fused(g, use, R, M, H, ld_pre=4 * H + 8, ld_x=M + 12)
        assert torch.equal(h, h2) and torch.equal(c, c2)


@pytest.mark.parametrize("M,H", [(20, 24), (512, 512)])
def test_lstm_step_rows_do_not_depend_on_the_batch_and_runs_are_identical(M, H):
    R = 65
    d = _inputs(R, M, H, seed=5)
    g = _dev(d)
    use = FORMS["x+h+bias"]
    h, c = _fused(g, use, R, M, H)
    h2, c2 = _fused(g, use, R, M, H)
    assert torch.equal(h, h2) and torch.equal(c, c2)  # two runs: the same bits
    for r in (0, 17, 63, 64):
        one = {k: (v[r:r + 1].contiguous() if k in ("x", "h", "c", "pre") else v) for k, v in g.items()}
        h1, c1 = _fused(one, use, 1, M, H)
        assert torch.equal(h1[0], h[r]) and torch.equal(c1[0], c[r]), r


def test_lstm_step_rejects_bad_arguments_without_launching():
    from capmi import kernels as K
    from capmi._lib import CapmiError
    R, M, H = 2, 16, 8
    g = _dev(_inputs(R, M, H))
    h_out, c_out = torch.full((R, H), 9.0, device=DEV), torch.full((R, H), 9.0, device=DEV)
    kw = dict(x=g["x"], h_prev=g["h"], c_prev=g["c"], w_ih=g["w_ih"], w_hh=g["w_hh"])
    with pytest.raises(CapmiError, match=str(EINVAL)):  # M % 4 != 0
        K.lstm_step_fwd(R, 14, H, h_out, c_out, **dict(kw, w_ih=g["w_ih"][:, :14].contiguous(), ld_x=16))
    with pytest.raises(CapmiError, match=str(EINVAL)):  # none of pre / x / h_prev
        K.lstm_step_fwd(R, M, H, h_out, c_out, c_prev=g["c"])
    with pytest.raises(CapmiError, match=str(EINVAL)):  # h_out == h_prev
        K.lstm_step_fwd(R, M, H, g["h"], c_out, **kw)
    torch.cuda.synchronize()
    assert (h_out == 9.0).all() and (c_out == 9.0).all()


# ---------------------------------------------------------------------------------------------------
# capmi_eval_rows_at
# ---------------------------------------------------------------------------------------------------
def _rows_at(x, caps, lens, tgt_off, entry="at"):
    from capmi import kernels as K
    B, T, V = x.shape
    L = caps.shape[1]
    xd, cd = t(x, DEV), t(caps, DEV)
    ld = None if lens is None else torch.tensor(lens, dtype=I32, device=DEV)
    loss = torch.full((B * T,), 123.0, device=DEV)
    pred = torch.full((B * T,), 77, dtype=I32, device=DEV)
    rank = torch.full((B * T,), 77, dtype=I32, device=DEV)
    if entry == "at":
        K.eval_rows_at(xd, cd, B, T, L, V, tgt_off, ld, loss, pred, rank)
    else:
        K.eval_rows(xd, cd, B, T, L, V, ld, loss, pred, rank)
    torch.cuda.synchronize()
    return loss.cpu().view(B, T), pred.cpu().view(B, T), rank.cpu().view(B, T)


def _check_rows_at(x, caps, lens, tgt_off):
    loss, pred, rank = _rows_at(x, caps, lens, tgt_off)
    wl, wp, wr = BC.rows_ref(x, caps, lens, tgt_off)
    assert np.array_equal(pred.numpy(), wp), (pred, wp)
    assert np.array_equal(rank.numpy(), wr), (rank, wr)
    for g, w in zip(loss.double().numpy().ravel(), wl.ravel()):
        assert (math.isinf(w) and g == w) or _close(g, w), (g, w)


@pytest.mark.parametrize("B,T,V", EC.ROW_SHAPES)
@pytest.mark.parametrize("ragged", [False, True])
def test_eval_rows_at_offset_0_matches_fp64(B, T, V, ragged):
    """The baseline layout: L = T, the target of step t is caps[b, t]. Constructed ties are exact."""
    x, caps = EC.constructed(B, T, V, seed=11, L=T + 1)
    caps = np.ascontiguousarray(caps[:, 1:])  # the planted targets move to column t
    assert caps.shape[1] == T
    _check_rows_at(x, caps, EC.ragged_lens(B, T) if ragged else None, 0)


def test_eval_rows_at_offset_1_is_eval_rows_bit_for_bit():
    for (B, T, V) in ((3, 3, 257), (1, 2, 8100)):
        x, caps = EC.constructed(B, T, V, seed=12, L=T + 3)
        for lens in (None, [T, 1, 0][:B]):
            a = _rows_at(x, caps, lens, 1)
            b = _rows_at(x, caps, lens, 1, entry="rows")
            for u, v in zip(a, b):
                assert torch.equal(u, v)


def test_eval_rows_at_offset_2_and_the_length_check():
    from capmi import kernels as K
    from capmi._lib import CapmiError
    B, T, V = 3, 3, 260
    x, caps = EC.constructed(B, T, V, seed=13, L=T + 2)
    _check_rows_at(x, caps, [1, 3, 2], 2)
    xd, cd = t(x, DEV), t(np.ascontiguousarray(caps[:, :T + 1]), DEV)
    out = [torch.zeros(B * T, device=DEV), torch.zeros(B * T, dtype=I32, device=DEV)]
    with pytest.raises(CapmiError, match=str(EINVAL)):  # L = T + 1 < T + 2
        K.eval_rows_at(xd, cd, B, T, T + 1, V, 2, None, out[0], out[1])


# ---------------------------------------------------------------------------------------------------
# capmi_eval_captions_ce
# ---------------------------------------------------------------------------------------------------
def test_eval_captions_ce_matches_fp64_and_is_deterministic():
    from capmi import kernels as K
    B, T = 4, 4
    lens = [4, 2, 0, 1]
    rng = np.random.default_rng([22])
    loss_rows = rng.uniform(0.5, 6.0, size=(B, T)).astype(np.float32)
    rank = rng.integers(0, 9, size=(B, T)).astype(np.int32)
    rank[0, :3] = [0, 4, 5]
    for b, n in enumerate(lens):  # junk past each length
        loss_rows[b, n:] = 1e6
        rank[b, n:] = 0
    want = EC.captions_ref(loss_rows, rank, np.zeros((B, T, 1)), lens)
    runs = []
    for _ in range(2):
        ce = torch.full((B,), -5.0, device=DEV)
        c = [torch.full((B,), -5, dtype=I32, device=DEV) for _ in range(2)]
        K.eval_captions_ce(t(loss_rows, DEV).view(-1), t(rank, DEV).view(-1), torch.tensor(lens, dtype=I32, device=DEV),
                           B, T, ce, c[0], c[1])
        torch.cuda.synchronize()
        runs.append([ce.cpu(), c[0].cpu(), c[1].cpu()])
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    ce, top1, top5 = runs[0]
    for b in range(B):
        assert _close(float(ce[b]), want["ce"][b]), (b, ce[b], want["ce"][b])
    assert top1.tolist() == want["top1"].tolist() and top5.tolist() == want["top5"].tolist()
    assert float(ce[2]) == 0.0 and top1[2] == 0 and top5[2] == 0
