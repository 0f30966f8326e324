"""GPU: the encoder's memory-bound kernels (csrc/encoder.hip, csrc/encoder_bwd.hip, the elementwise tail of
csrc/gemm_bf16.hip), each against a plain fp64 reference of the same operation at the shapes where its
code takes another path: one slab and 256, a partial last slab, the finalize lanes' second trip, a partly
filled channel block, H != W, odd maps, every grid cap passed, in-place and accumulate forms.

Cases, references and comparison rules live in tests/encoder_kernel_cases.py (pinned themselves by
tests/test_encoder_kernel_cases_cpu.py); the references run in fp64 on the device from the very fp32 / bf16
tensors the kernel gets. Every output is a view into a NaN-filled buffer with 64-float guard zones on both
sides: after the call the guards are still NaN and the output holds none."""
import math

import pytest
import torch

import encoder_kernel_cases as EC
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _K():
    from capmi import kernels as K
    return K


class Guarded:
    """A NaN-filled buffer; ``v`` is the 16-byte aligned view of ``shape`` between two guard zones of 256 B
    (64 floats)."""

    def __init__(self, shape, dtype=torch.float32):
        self.g = 256 // torch.empty(0, dtype=dtype).element_size()
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * self.g,), NAN, dtype=dtype, device=DEV)
        self.v = self.buf[self.g:self.g + self.n].view(shape)
        assert self.v.data_ptr() % 16 == 0

    def check(self, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:self.g]).all()) and bool(torch.isnan(self.buf[self.g + self.n:]).all()), \
            f"{what}: wrote outside its output"
        assert not bool(torch.isnan(self.v).any()), f"{what}: left part of its output unwritten (or wrote NaN)"
        return self.v

    def untouched(self, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf).all()), f"{what}: wrote although it rejected the call"


def dev(p):
    return {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in p.items()}


# ------------------------------------------------------------------------------------------ BN backward
def bn_args(mode, p):
    """(mask_src, scale, shift) as the fine-tune backward passes them in ``mode``."""
    return (None, p["scale"], p["shift"]) if mode == 0 else (p["out"], None, None)


def run_reduce(mode, p, accumulate=False, old=None):
    K = _K()
    C = p["C"]
    dg, db, coef = Guarded((C,)), Guarded((C,)), Guarded((4 * C,))
    if old is not None:
        dg.v.copy_(old[0])
        db.v.copy_(old[1])
    work = torch.full((K.bnb_work_floats(C),), NAN, device=DEV)
    m, sc, sh = bn_args(mode, p)
    K.bn_bwd_reduce(mode, p["d"], p["y"], m, sc, sh, p["gamma"], p["mean"], p["var"], p["eps"], p["rows"], C,
                    dg.v, db.v, coef.v, work, accumulate=accumulate)
    return dg.check("bn_bwd_reduce dgamma"), db.check("bn_bwd_reduce dbeta"), coef.check("bn_bwd_reduce coef")


def run_apply(mode, p, coef, d=None, dy=None, with_dz=None):
    """bn_bwd_apply into guarded outputs; ``dy`` = a Guarded holding d runs it in place."""
    K = _K()
    rows, C = p["rows"], p["C"]
    with_dz = (mode == 1) if with_dz is None else with_dz
    dy = Guarded((rows, C)) if dy is None else dy
    dz = Guarded((rows, C)) if with_dz else None
    m, sc, sh = bn_args(mode, p)
    K.bn_bwd_apply(mode, p["d"] if d is None else d, p["y"], m, sc, sh, coef, rows, C, dy.v, dz.v if dz else None)
    return dy.check("bn_bwd_apply dy"), (dz.check("bn_bwd_apply dz_out") if dz else None)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,C", EC.BN_CASES)
def test_bn_backward(rows, C, mode):
    """bn_bwd_reduce + bn_bwd_finalize_kernel + bn_bwd_apply at every slab plan of EC.BN_CASES: dgamma, dbeta and
    coef against the fp64 closed form (the mask formed exactly, so no ReLU decision is in doubt); the apply on
    its own against the closed form evaluated from the coef the GPU produced; and the end-to-end relative-L2
    bound of 1e-5 against fp64 autograd of F.batch_norm(training=True)."""
    p = dev(EC.bn_inputs(rows, C))
    ref = EC.bn_bwd_ref(mode, p)
    what = f"bn_bwd ({rows}, {C}) mode {mode}"
    dg, db, coef = run_reduce(mode, p)
    EC.check_bn_reduce(dg, db, coef, p, ref, f"{what} reduce")
    dy, dz = run_apply(mode, p, coef)
    want, mag = EC.bn_apply_ref(ref["dz"], p["y"], coef)
    EC.within(dy, want, mag, f"{what} apply dy")
    if mode == 1:
        EC.exact(dz, ref["dz"].float(), f"{what} apply dz_out")
    ady, adg, adb = EC.bn_bwd_autograd(dev_cpu(p), ref["dz"].cpu())
    errs = rel_err(dy, ady), rel_err(dg, adg), rel_err(db, adb)
    print(f"{what} vs autograd: rel L2 dy {errs[0]:.3g} dgamma {errs[1]:.3g} dbeta {errs[2]:.3g}")
    assert max(errs) < 1e-5, errs


def dev_cpu(p):
    return {k: v.cpu() if torch.is_tensor(v) else v for k, v in p.items()}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,C", EC.BN_EXTRA_CASES)
def test_bn_backward_accumulate_and_determinism(rows, C, mode):
    """accumulate=1 adds onto what dgamma / dbeta hold (and coef is the plain call's); two runs of one call
    agree bit for bit (the fixed-shape LDS tree of the finalize)."""
    p = dev(EC.bn_inputs(rows, C))
    what = f"bn_bwd ({rows}, {C}) mode {mode}"
    dg, db, coef = run_reduce(mode, p)
    dg2, db2, coef2 = run_reduce(mode, p)
    for a, b, n in ((dg, dg2, "dgamma"), (db, db2, "dbeta"), (coef, coef2, "coef")):
        EC.exact(b, a, f"{what} second run {n}")
    old = EC.bn_eval_inputs(C)[0].to(DEV), EC.bn_eval_inputs(C)[1].to(DEV) + 0.75
    adg, adb, acoef = run_reduce(mode, p, accumulate=True, old=old)
    for got, o, plain, n in ((adg, old[0], dg, "dgamma"), (adb, old[1], db, "dbeta")):
        EC.within(got, o.double() + plain.double(), o.double().abs() + plain.double().abs(),
                  f"{what} accumulate {n}")
    EC.exact(acoef, coef, f"{what} accumulate coef")


@pytest.mark.parametrize("rows,C", EC.BN_EXTRA_CASES)
def test_bn_apply_production_forms(rows, C):
    """The forms the fine-tune backward calls: mode 0 in place (dy is d), and the bottleneck tail (mode 1)
    with dz_out set and without: each bit-identical to the out-of-place result."""
    p = dev(EC.bn_inputs(rows, C))
    _, _, coef = run_reduce(0, p)
    dy, _ = run_apply(0, p, coef)
    inplace = Guarded((rows, C))
    inplace.v.copy_(p["d"])
    got, _ = run_apply(0, p, coef, d=inplace.v, dy=inplace)
    EC.exact(got, dy, f"bn_bwd_apply ({rows}, {C}) in place")
    _, _, coef = run_reduce(1, p)
    dy, _ = run_apply(1, p, coef, with_dz=False)
    got, dz = run_apply(1, p, coef, with_dz=True)
    EC.exact(got, dy, f"bn_bwd_apply ({rows}, {C}) tail with dz_out")
    EC.exact(dz, EC.bn_dz(1, p).float(), f"bn_bwd_apply ({rows}, {C}) tail dz_out")


def test_bn_apply_past_the_grid_cap():
    """rows * C / 4 > 16384 * 256 float4: the apply's grid-stride loop takes a second trip. Mode 0, in place,
    the coef from a reduce on the same data (249 slabs over 8 channel blocks)."""
    rows, C = EC.BN_APPLY_BIG
    p = dev(EC.bn_inputs(rows, C))
    ref = EC.bn_bwd_ref(0, p)
    dg, db, coef = run_reduce(0, p)
    EC.check_bn_reduce(dg, db, coef, p, ref, f"bn_bwd ({rows}, {C}) reduce")
    want, mag = EC.bn_apply_ref(ref["dz"], p["y"], coef)
    del ref
    inplace = Guarded((rows, C))
    inplace.v.copy_(p["d"])
    got, _ = run_apply(0, p, coef, d=inplace.v, dy=inplace)
    EC.within(got, want, mag, f"bn_bwd_apply ({rows}, {C}) in place past the grid cap")


# ------------------------------------------------------------------------------------------ conv1 tail
@pytest.mark.parametrize("N,H,W,C", EC.MAXPOOL_CASES)
def test_bn_relu_maxpool(N, H, W, C):
    """maxpool3x3/2/p1(relu(fma(y, s, b))): one fp32 rounding (relu and max add none) of a value no larger
    than the window maximum of |y||s| + |b|."""
    K = _K()
    y, s, b = (v.to(DEV) for v in EC.maxpool_inputs(N, H, W, C))
    Ho, Wo = EC.maxpool_out(H, W)
    out = Guarded((N, Ho, Wo, C))
    K.bn_relu_maxpool(y, s, b, out.v, N, H, W, C, Ho, Wo)
    got = out.check("bn_relu_maxpool")
    ref, mag = EC.maxpool_ref(y, s, b)
    EC.one_rounding(got, ref, mag, f"bn_relu_maxpool {(N, H, W, C)}")
    assert float(got[..., C - 1].abs().max()) == 0.0  # the all-negative channel: zeros, never -inf


# ------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("case", EC.POOL_CASES, ids=EC.case_id)
def test_adaptive_avgpool_nhwc(case):
    K = _K()
    N, H, W, OH, OW, C = case
    x = EC.pool_inputs(*case)[0].to(DEV)
    out = Guarded((N, OH, OW, C))
    K.adaptive_avgpool_nhwc(x, N, H, W, C, OH, OW, out.v)
    got = out.check("adaptive_avgpool_nhwc")
    if case in EC.POOL_GATHER_CASES:  # one-pixel windows: x + 0, times 1
        EC.exact(got, EC.pool_gather(x, OH, OW), f"adaptive_avgpool_nhwc {case}")
    ref, mag = EC.pool_fwd_ref(x, OH, OW)
    EC.within(got, ref, mag, f"adaptive_avgpool_nhwc {case}")


@pytest.mark.parametrize("case", EC.POOL_CASES, ids=EC.case_id)
def test_adaptive_avgpool_bf16(case):
    """The bf16-input pool: exact bf16 inputs, fp32 accumulation, so the fp32 rule holds."""
    K = _K()
    N, H, W, OH, OW, C = case
    x = EC.pool_inputs(*case, dtype=EC.BF)[0].to(DEV)
    out = Guarded((N, OH, OW, C))
    K.adaptive_avgpool_bf16(x, N, H, W, C, OH, OW, out.v)
    got = out.check("adaptive_avgpool_bf16")
    if case in EC.POOL_GATHER_CASES:
        EC.exact(got, EC.pool_gather(x, OH, OW).float(), f"adaptive_avgpool_bf16 {case}")
    ref, mag = EC.pool_fwd_ref(x, OH, OW)
    EC.within(got, ref, mag, f"adaptive_avgpool_bf16 {case}")


@pytest.mark.parametrize("case", EC.POOL_CASES, ids=EC.case_id)
def test_adaptive_avgpool_bwd_nhwc(case):
    K = _K()
    N, H, W, OH, OW, C = case
    d = EC.pool_inputs(*case)[1].to(DEV)
    din = Guarded((N, H, W, C))
    K.adaptive_avgpool_bwd_nhwc(d, N, H, W, C, OH, OW, din.v)
    got = din.check("adaptive_avgpool_bwd_nhwc")
    ref, mag = EC.pool_bwd_ref(d, H, W)
    EC.within(got, ref, mag, f"adaptive_avgpool_bwd_nhwc {case}")
    if (H, W) == (OH, OW):
        EC.exact(got, d, f"adaptive_avgpool_bwd_nhwc {case} identity")


# ------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("co,ci,kh,kw,cp", EC.PACK_CASES)
def test_conv_weight_pack_pad(co, ci, kh, kw, cp):
    K = _K()
    w = EC.weights(co, ci, kh, kw).to(DEV)
    out = Guarded((co, kh, kw, cp))
    K.conv_weight_pack_pad(w, cp, out.v)
    EC.exact(out.check("conv_weight_pack_pad"), EC.pack_pad_ref(w, cp), f"conv_weight_pack_pad {(co, ci, kh, kw, cp)}")
    out = Guarded((co, kh, kw, ci))
    K.conv_weight_pack(w, out.v)
    EC.exact(out.check("conv_weight_pack"), EC.pack_pad_ref(w, ci), f"conv_weight_pack {(co, ci, kh, kw)}")


@pytest.mark.parametrize("co,ci,kh,kw,cp", EC.PACK_CASES)
def test_conv_weight_pack_dgrad_and_unpack(co, ci, kh, kw, cp):
    K = _K()
    w = EC.weights(co, ci, kh, kw).to(DEV)
    out = Guarded((ci, kh, kw, co))
    K.conv_weight_pack_dgrad(w, out.v)
    EC.exact(out.check("conv_weight_pack_dgrad"), EC.pack_dgrad_ref(w), f"conv_weight_pack_dgrad {(co, ci, kh, kw)}")
    # unpack of an arbitrary [Cout][KH][KW][Cin] buffer, then the round trip through the forward pack
    g = EC.weights(co, kh * kw, ci, 1).to(DEV).reshape(-1)
    back = Guarded((co, ci, kh, kw))
    K.conv_weight_unpack(g, (co, ci, kh, kw), back.v)
    EC.exact(back.check("conv_weight_unpack"), EC.unpack_ref(g, (co, ci, kh, kw)), f"conv_weight_unpack {(co, ci, kh, kw)}")
    packed = torch.empty(co, kh, kw, ci, device=DEV)
    K.conv_weight_pack(w, packed)
    back = Guarded((co, ci, kh, kw))
    K.conv_weight_unpack(packed, (co, ci, kh, kw), back.v)
    EC.exact(back.check("conv_weight_unpack"), w, f"unpack(pack(w)) {(co, ci, kh, kw)}")


@pytest.mark.parametrize("ph,pw", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("co,ci", EC.PACK_S2_CASES)
def test_conv_weight_pack_dgrad_s2(co, ci, ph, pw):
    K = _K()
    w = EC.weights(co, ci, 3, 3).to(DEV)
    out = Guarded((ci, ph + 1, pw + 1, co))
    K.conv_weight_pack_dgrad_s2(w, ph, pw, out.v)
    EC.exact(out.check("conv_weight_pack_dgrad_s2"), EC.pack_dgrad_s2_ref(w, ph, pw),
             f"conv_weight_pack_dgrad_s2 {(co, ci)} class {(ph, pw)}")


@pytest.mark.parametrize("N,C,H,W", EC.IMAGE_CASES)
def test_image_nhwc4(N, C, H, W):
    K = _K()
    g = torch.Generator().manual_seed(N + 10 * C + 100 * H + 1000 * W)
    if N == 0:  # accepted, and nothing is written (an empty torch tensor has no pointer: the entry point itself)
        imgs, out = EC._u(g, (1, C, H, W)).to(DEV), Guarded((1, H, W, 4))
        K.call("capmi_image_nhwc4", K.ptr(imgs), 0, C, H, W, K.ptr(out.v), K.stream())
        out.untouched("image_nhwc4 N=0")
        return
    imgs = EC._u(g, (N, C, H, W)).to(DEV)
    out = Guarded((N, H, W, 4))
    K.image_nhwc4(imgs, out.v)
    EC.exact(out.check("image_nhwc4"), EC.image_nhwc4_ref(imgs), f"image_nhwc4 {(N, C, H, W)}")


@pytest.mark.parametrize("Ho,Wo,H,W", EC.UPSAMPLE_CASES)
def test_zero_upsample2_nhwc(Ho, Wo, H, W):
    K = _K()
    N, C = 2, 8
    g = torch.Generator().manual_seed(Ho + 10 * Wo + 100 * H + 1000 * W)
    dy = (EC._u(g, (N, Ho, Wo, C)) + 1.5).to(DEV)  # (no zero among the copied values)
    out = Guarded((N, H, W, C))
    K.zero_upsample2_nhwc(dy, N, Ho, Wo, C, H, W, out.v)
    EC.exact(out.check("zero_upsample2_nhwc"), EC.zero_upsample2_ref(dy, H, W), f"zero_upsample2_nhwc {(Ho, Wo, H, W)}")


@pytest.mark.parametrize("C", EC.BN_EVAL_CASES)
def test_bn_eval_params(C):
    K = _K()
    gamma, beta, rm, rv = (v.to(DEV) for v in EC.bn_eval_inputs(C))
    eps = float(torch.tensor(EC.EPS, dtype=torch.float32))
    scale, shift = Guarded((C,)), Guarded((C,))
    K.bn_eval_params(gamma, beta, rm, rv, C, eps, scale.v, shift.v)
    rs, rb, ms, mb = EC.bn_eval_ref(gamma, beta, rm, rv, eps)
    EC.within(scale.check("bn_eval_params scale"), rs, ms, f"bn_eval_params scale C={C}")
    EC.within(shift.check("bn_eval_params shift"), rb, mb, f"bn_eval_params shift C={C}")


# ------------------------------------------------------------------------------------------ bf16 BN kernels
@pytest.mark.parametrize("rows,C", EC.BF16_CASES)
def test_bf16_bn_kernels(rows, C):
    """bn_relu_bf16 bit for bit (one fma, one RNE rounding); bn_add_relu_bf16 with the identity and the
    downsample-BN residual within half a bf16 ulp plus the fp32 roundings before it. At (131075, 64) the
    grid-stride loop takes a second trip on threads 0..23, which must still hold their channel group."""
    K = _K()
    y, r, s, b, rs, rb = (v.to(DEV) for v in EC.bf16_inputs(rows, C))
    x = Guarded((rows, C), EC.BF)
    K.bn_relu_bf16(y, s, b, rows, C, x.v)
    EC.exact(x.check("bn_relu_bf16"), EC.bn_relu_bf16_ref(y, s, b), f"bn_relu_bf16 {(rows, C)}")
    for extra, name in (((), "identity residual"), ((rs, rb), "residual BN")):
        out = Guarded((rows, C), EC.BF)
        K.bn_add_relu_bf16(y, s, b, r, out.v, rows, C, *extra)
        ref, mag = EC.bn_add_relu_bf16_ref(y, s, b, r, *extra)
        EC.bf16_rounded(out.check("bn_add_relu_bf16"), ref, mag, f"bn_add_relu_bf16 {(rows, C)} {name}")


# ------------------------------------------------------------------------------------------ rejections
def rejected(what, out, fn, *a, **kw):
    from capmi import CapmiError
    with pytest.raises(CapmiError):
        fn(*a, **kw)
    for o in out:
        o.untouched(what)


def test_argument_rejections():
    """Every entry point validates before any launch: the call raises CapmiError and the NaN-filled output
    stays NaN."""
    K = _K()
    rows, C = 16, 8
    f = lambda *shape: torch.ones(*shape, device=DEV)  # noqa: E731
    o = Guarded((rows, C))
    # C = 6 (not a multiple of 4)
    rejected("bn_add_relu C=6", [o], K.bn_add_relu, f(rows, 6), f(8), f(8), f(rows, 6), o.v, rows, 6)
    dg, db, coef = Guarded((C,)), Guarded((C,)), Guarded((4 * C,))
    work = torch.empty(K.bnb_work_floats(C), device=DEV)

    def red(mode, m, sc, sh, c=C):
        K.bn_bwd_reduce(mode, f(rows, C), f(rows, C), m, sc, sh, f(C), f(C), f(C), 1e-5, rows, c, dg.v, db.v, coef.v,
                        work)

    rejected("bn_bwd_reduce C=6", [dg, db, coef], red, 0, None, f(C), f(C), 6)
    rejected("bn_bwd_reduce mode 1 without mask_src", [dg, db, coef], red, 1, None, None, None)
    rejected("bn_bwd_reduce mode 0 without scale", [dg, db, coef], red, 0, None, None, f(C))
    mp = Guarded((1, 2, 2, 8))
    rejected("bn_relu_maxpool C=6", [mp], K.bn_relu_maxpool, f(1, 4, 4, 8), f(8), f(8), mp.v, 1, 4, 4, 6, 2, 2)
    rejected("bn_relu_maxpool Ho one too large", [mp], K.bn_relu_maxpool, f(1, 2, 4, 8), f(8), f(8), mp.v, 1, 2, 4, 8,
             2, 2)
    # a view offset by one float as y
    off = torch.ones(rows * C + 4, device=DEV)[1:1 + rows * C].view(rows, C)
    assert off.data_ptr() % 16 == 4
    rejected("bn_bwd_apply misaligned y", [o], K.bn_bwd_apply, 0, f(rows, C), off, None, f(C), f(C), f(4 * C), rows, C,
             o.v)
    po = Guarded((1, 2, 2, 8))
    offp = torch.ones(4 * 4 * 8 + 4, device=DEV)[1:1 + 4 * 4 * 8]
    rejected("adaptive_avgpool_nhwc misaligned input", [po], K.adaptive_avgpool_nhwc, offp, 1, 4, 4, 8, 2, 2, po.v)
    up = Guarded((2, 4, 8, 8))
    rejected("zero_upsample2_nhwc H = 2 Ho - 2", [up], K.zero_upsample2_nhwc, f(2, 3, 4, 8), 2, 3, 4, 8, 4, 8, up.v)
    xb = Guarded((rows, 24), EC.BF)
    yb = torch.ones(rows, 24, device=DEV, dtype=EC.BF)
    rejected("bn_relu_bf16 C=24", [xb], K.bn_relu_bf16, yb, f(24), f(24), rows, 24, xb.v)
