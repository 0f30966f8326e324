"""CPU: the references and comparison rules of the encoder non-GEMM kernel tests
(tests/encoder_kernel_cases.py, which tests/test_gpu_encoder_kernels.py runs the kernels against).

  * the closed-form BN backward is anchored to fp64 autograd through F.batch_norm(training=True);
  * the case inputs leave headroom: an fp32 emulation of each kernel's arithmetic passes its rule;
  * every rule has teeth: an emulation of a plausible kernel bug fails the very comparison the GPU test
    makes (a dropped slab, the finalize's second trip lost, accumulate ignored, H and W swapped in a pool,
    a max-pool row past the image read, kh and kw swapped in a pack, a bf16 thread on the next channel
    group).

The argument rejections stay in the GPU file: the entry points do validate before they touch the device, but
driving them from here needs stand-in pointers, and a validation that ever regressed would then launch on
them on a machine that has a GPU."""
import pytest
import torch

import encoder_kernel_cases as EC
from helpers import rel_err


@pytest.fixture(scope="module")
def bn():
    """(inputs, {mode: fp64 reference}) per BN case, computed once."""
    cache = {}

    def get(rows, C):
        if (rows, C) not in cache:
            p = EC.bn_inputs(rows, C)
            cache[(rows, C)] = (p, {m: EC.bn_bwd_ref(m, p) for m in (0, 1)})
        return cache[(rows, C)]
    return get


def fails(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


# ------------------------------------------------------------------------------------------ the plan
def test_slab_plan_is_the_table():
    """The comment table beside BN_CASES, and the paths the issue picked the shapes for."""
    for rows, C in EC.BN_CASES:
        assert EC.slab_plan(rows, C) == EC.BN_PLANS[(rows, C)], (rows, C)
    CB, gx, slabs, per = EC.slab_plan(545, 12)
    assert 256 % CB != 0 and slabs > EC.BNB_FIN_LANES and 545 - (slabs - 1) * per == 18
    assert EC.slab_plan(8192, 8)[2] == EC.BNB_MAX_SLABS
    assert 8197 - 248 * 33 == 13
    assert EC.slab_plan(31, 8)[3] < 256 // EC.slab_plan(31, 8)[0]
    assert EC.slab_plan(100, 320)[1] == 2 and (320 // 4) % 64 == 16
    rows, C = EC.BN_APPLY_BIG
    assert rows * C // 4 > 16384 * 256


# ------------------------------------------------------------------------------------------ a. the anchor
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,C", EC.BN_CASES)
def test_closed_form_is_autograd(bn, rows, C, mode):
    """The closed form from the fp32-rounded mean / var against fp64 autograd fed the same dz: relative L2
    1e-6 (measured about 1.5e-8, all of it the rounding of the saved statistics)."""
    p, refs = bn(rows, C)
    ref = refs[mode]
    dy, dg, db = EC.bn_bwd_autograd(p, ref["dz"])
    errs = rel_err(ref["dy"], dy), rel_err(ref["dgamma"], dg), rel_err(ref["dbeta"], db)
    print(f"closed form vs autograd ({rows}, {C}) mode {mode}: dy {errs[0]:.3g} dgamma {errs[1]:.3g} "
          f"dbeta {errs[2]:.3g}")
    assert max(errs) < 1e-6, errs
    # both ReLU branches are taken, so the mask matters
    frac = float(ref["mask"].double().mean())
    assert 0.05 < frac < 0.95, frac


# ------------------------------------------------------------------------------------------ b. headroom
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,C", EC.BN_CASES)
def test_bn_fp32_two_stage_sum_passes(bn, rows, C, mode):
    """Per-slab fp32 partials and an fp64 total pass every reduce rule, and the apply's rule from that coef."""
    p, refs = bn(rows, C)
    ref = refs[mode]
    dg, db, coef = EC.bn_bwd_emulate(mode, p)
    r = EC.check_bn_reduce(dg, db, coef, p, ref, f"emulated bn_bwd_reduce ({rows}, {C}) mode {mode}")
    assert max(v for k, v in r.items() if k != "coef0") < 0.5, r  # (one rounding reaches its bound: up to 1)
    # the apply in fp32 (two fmas and the subtraction of the mean) from the emulated coef
    c = coef.view(4, C)
    dz32 = ref["dz"].float()
    dy32 = EC.fma32(c[0], dz32, -EC.fma32(c[1], p["y"] - c[3], c[2]))
    want, mag = EC.bn_apply_ref(ref["dz"], p["y"], coef)
    assert EC.within(dy32, want, mag, f"emulated bn_bwd_apply ({rows}, {C}) mode {mode}") < 0.5


# ------------------------------------------------------------------------------------------ c. teeth
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,C", [(545, 12), (8197, 8), (392, 2048)])
def test_dropped_last_slab_fails(bn, rows, C, mode):
    p, refs = bn(rows, C)
    ref = refs[mode]
    dg, db, coef = EC.bn_bwd_emulate(mode, p, drop_last_slab=True)
    fails(EC.within, dg, ref["dgamma"], ref["mag_dg"], "dgamma without the last slab")
    fails(EC.within, db, ref["dbeta"], ref["mag_db"], "dbeta without the last slab")
    fails(EC.check_bn_reduce, dg, db, coef, p, ref, "reduce without the last slab")
    c = coef.view(4, C)
    fails(EC.within, c[1], ref["coef"][1], ref["mag_coef"][1], "coef1 without the last slab")
    fails(EC.within, c[2], ref["coef"][2], ref["mag_coef"][2], "coef2 without the last slab")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,C", [(545, 12), (8192, 8), (8197, 8)])
def test_lost_second_finalize_trip_fails(bn, rows, C, mode):
    """Slabs k >= 16 are the finalize lanes' second and later trips (k += 16)."""
    p, refs = bn(rows, C)
    ref = refs[mode]
    dg, db, coef = EC.bn_bwd_emulate(mode, p, max_slabs=EC.BNB_FIN_LANES)
    fails(EC.within, dg, ref["dgamma"], ref["mag_dg"], "dgamma of slabs 0..15")
    fails(EC.within, db, ref["dbeta"], ref["mag_db"], "dbeta of slabs 0..15")
    fails(EC.check_bn_reduce, dg, db, coef, p, ref, "reduce of slabs 0..15")


@pytest.mark.parametrize("rows,C", EC.BN_EXTRA_CASES)
def test_ignored_accumulate_fails(bn, rows, C):
    """The GPU test's accumulate check (old + plain, magnitude |old| + |plain|) rejects a plain store."""
    p, _ = bn(rows, C)
    dg, db, _ = EC.bn_bwd_emulate(0, p)
    old_g, old_b = EC.bn_eval_inputs(C)[0], EC.bn_eval_inputs(C)[1] + 0.75
    for plain, old, what in ((dg, old_g, "dgamma"), (db, old_b, "dbeta")):
        want, mag = old.double() + plain.double(), old.double().abs() + plain.double().abs()
        assert EC.within(old + plain, want, mag, f"accumulated {what}") < 0.1
        fails(EC.within, plain, want, mag, f"{what} with accumulate ignored")


def test_one_rounding_has_teeth(bn):
    """coef0 passes as the fp32 rounding of the fp64 value and fails one fp32 ulp away; two roundings (k1
    formed in fp32 from an fp32 invstd) fail somewhere among 2048 channels."""
    p, refs = bn(392, 2048)
    ref = refs[0]
    k1 = ref["coef"][0].float()
    assert EC.one_rounding(k1, ref["coef"][0], ref["mag_coef"][0], "coef0 rounded once") <= 1.0
    fails(EC.one_rounding, torch.nextafter(k1, k1 * 2), ref["coef"][0], ref["mag_coef"][0], "coef0 one ulp up")
    inv32 = (1.0 / torch.sqrt(p["var"].double() + p["eps"])).float()
    fails(EC.one_rounding, p["gamma"] * inv32, ref["coef"][0], ref["mag_coef"][0], "coef0 rounded twice")


@pytest.mark.parametrize("N,H,W,C", [c for c in EC.MAXPOOL_CASES if c[1] * c[2] <= 112 * 112])
def test_maxpool_emulation_passes(N, H, W, C):
    y, s, b = EC.maxpool_inputs(N, H, W, C)
    ref, mag = EC.maxpool_ref(y, s, b)
    got = EC.maxpool_emulate(y, s, b)
    assert got.shape == ref.shape == (N,) + EC.maxpool_out(H, W) + (C,)
    assert EC.one_rounding(got, ref, mag, f"emulated bn_relu_maxpool {(N, H, W, C)}") <= 1.0
    assert float(ref[..., C - 1].abs().max()) == 0.0 and bool(torch.isfinite(got).all())
    assert float(ref[..., :C - 1].max()) > 0.0


def test_maxpool_row_past_the_image_fails():
    """Odd H: the last output row's window reaches ih = H, the next image's first row."""
    N, H, W, C = EC.MAXPOOL_CASES[0]
    assert H % 2 == 1 and N > 1
    y, s, b = EC.maxpool_inputs(N, H, W, C)
    ref, mag = EC.maxpool_ref(y, s, b)
    fails(EC.one_rounding, EC.maxpool_emulate(y, s, b, skip_row_past_end=False), ref, mag, "row H not skipped")


@pytest.mark.parametrize("case", [c for c in EC.POOL_CASES if c[0] == 2], ids=EC.case_id)
def test_pool_emulation_passes(case):
    N, H, W, OH, OW, C = case
    x, d = EC.pool_inputs(*case)
    ref, mag = EC.pool_fwd_ref(x, OH, OW)
    got = EC._nhwc(torch.nn.functional.adaptive_avg_pool2d(EC._nchw(x), (OH, OW)))
    assert EC.within(got, ref, mag, f"fp32 pool {case}") < 0.1
    if case in EC.POOL_GATHER_CASES:
        EC.exact(got, EC.pool_gather(x, OH, OW), f"fp32 pool {case} is a gather")
    g, gm = EC.pool_bwd_ref(d, H, W)
    xx = EC._nchw(x).clone().requires_grad_()
    torch.nn.functional.adaptive_avg_pool2d(xx, (OH, OW)).backward(EC._nchw(d))
    assert EC.within(EC._nhwc(xx.grad), g, gm, f"fp32 pool backward {case}") < 0.1


@pytest.mark.parametrize("case", [c for c in EC.POOL_CASES if c[0] == 2 and c[1] != c[2]], ids=EC.case_id)
def test_pool_hw_swap_fails(case):
    N, H, W, OH, OW, C = case
    x, d = EC.pool_inputs(*case)
    ref, mag = EC.pool_fwd_ref(x, OH, OW)
    fails(EC.within, EC.pool_fwd_swapped(x, OH, OW), ref, mag, "forward pool, H and W swapped")
    g, gm = EC.pool_bwd_ref(d, H, W)
    fails(EC.within, EC.pool_bwd_swapped(d, H, W), g, gm, "backward pool, H and W swapped")
    # the bf16-input pool goes through the same rule
    xb = x.to(EC.BF)
    ref, mag = EC.pool_fwd_ref(xb, OH, OW)
    fails(EC.within, EC.pool_fwd_swapped(xb, OH, OW), ref, mag, "bf16 pool, H and W swapped")


def test_pool_cases_cover_what_they_claim():
    assert [c for c in EC.POOL_GATHER_CASES] == [EC.POOL_CASES[i] for i in (0, 1, 5, 6, 7)]
    N, H, W, OH, OW, C = EC.POOL_CASES[-1]
    assert N * OH * OW * C // 4 > 8192 * 256
    N, H, W, C = EC.MAXPOOL_CASES[-1]
    Ho, Wo = EC.maxpool_out(H, W)
    assert N * Ho * Wo * C // 4 > 8192 * 256
    co, ci, kh, kw, cp = EC.PACK_CASES[-1]
    assert co * cp * kh * kw > 8192 * 256
    rows, C = EC.BF16_CASES[-1]
    assert 0 < rows * C // 8 - 4096 * 256 < 256 and (4096 * 256) % (C // 8) == 0
    for rows, C in EC.BF16_CASES:
        assert C % 8 == 0 and 256 % (C // 8) == 0


@pytest.mark.parametrize("co,ci,kh,kw,cp", EC.PACK_CASES[:4])
def test_pack_references_and_khkw_swap(co, ci, kh, kw, cp):
    """The layout references against index loops written out, and a kh / kw swap failing exact."""
    w = EC.weights(co, ci, kh, kw)
    pad, dg = EC.pack_pad_ref(w, cp), EC.pack_dgrad_ref(w)
    assert pad.shape == (co, kh, kw, cp) and dg.shape == (ci, kh, kw, co)
    g = torch.Generator().manual_seed(1)
    for _ in range(64):
        o, i, h, v = (int(torch.randint(0, n, (1,), generator=g)) for n in (co, ci, kh, kw))
        assert pad[o, h, v, i] == w[o, i, h, v]
        assert dg[i, h, v, o] == w[o, i, kh - 1 - h, kw - 1 - v]
    assert cp == ci or float(pad[..., ci:].abs().max()) == 0.0
    packed = EC.pack_pad_ref(w, ci)
    EC.exact(EC.unpack_ref(packed.reshape(-1), w.shape), w, "unpack(pack(w))")
    if min(kh, kw) == 1:  # a unit extent: the swapped layout is the same buffer
        EC.exact(EC.pack_pad_khkw_swapped(w, cp).reshape(-1), pad.reshape(-1), "1 x k pack_pad, kh and kw swapped")
        fails(EC.exact, w.permute(1, 2, 3, 0).contiguous(), dg, "pack_dgrad without the flip")
    else:
        fails(EC.exact, EC.pack_pad_khkw_swapped(w, cp), pad, "pack_pad, kh and kw swapped")
        fails(EC.exact, EC.pack_dgrad_khkw_swapped(w), dg, "pack_dgrad, kh and kw swapped")
        fails(EC.exact, EC.unpack_khkw_swapped(packed.reshape(-1), w.shape), w, "unpack, kh and kw swapped")


def test_pack_khkw_swap_fails_on_square_kernels_too():
    co, ci, kh, kw, cp = EC.PACK_CASES[0]
    w = EC.weights(co, ci, kh, kw)
    fails(EC.exact, EC.pack_pad_khkw_swapped(w, cp), EC.pack_pad_ref(w, cp), "7x7 pack_pad, kh and kw swapped")
    fails(EC.exact, EC.pack_dgrad_khkw_swapped(w), EC.pack_dgrad_ref(w), "7x7 pack_dgrad, kh and kw swapped")


@pytest.mark.parametrize("ph,pw", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pack_dgrad_s2_reference(ph, pw):
    """The sub-pixel class (ph, pw) of a 3x3 / stride-2 / pad-1 conv's data gradient: input pixel
    (2i + ph, 2j + pw) gets dY[i + th][j + tw] * W[kh(th)][kw(tw)]; checked against autograd of the conv."""
    co, ci = EC.PACK_S2_CASES[0]
    w = EC.weights(co, ci, 3, 3).double()
    p = EC.pack_dgrad_s2_ref(w, ph, pw)
    assert p.shape == (ci, ph + 1, pw + 1, co)
    x = torch.zeros(1, ci, 8, 8, dtype=torch.float64, requires_grad=True)
    g = torch.Generator().manual_seed(5)
    dy = torch.rand(1, co, 4, 4, generator=g, dtype=torch.float64)
    torch.nn.functional.conv2d(x, w, stride=2, padding=1).backward(dy)
    dyp = torch.nn.functional.pad(dy, (0, 1, 0, 1))
    for i in range(4):
        for j in range(4):
            want = x.grad[0, :, 2 * i + ph, 2 * j + pw]
            got = sum(p[:, th, tw] @ dyp[0, :, i + th, j + tw] for th in range(ph + 1) for tw in range(pw + 1))
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    if ph != pw:
        other = EC.pack_dgrad_s2_ref(w, pw, ph)
        assert other.shape != p.shape  # a (ph, pw) mix-up changes the very size


def test_image_and_upsample_references():
    for N, C, H, W in EC.IMAGE_CASES:
        imgs = torch.arange(N * C * H * W, dtype=torch.float32).view(N, C, H, W) + 1
        o = EC.image_nhwc4_ref(imgs)
        assert o.shape == (N, H, W, 4)
        if N:
            assert o[N - 1, H - 1, 0, C - 1] == imgs[N - 1, C - 1, H - 1, 0] and float(o[..., C:].abs().sum()) == 0
    for Ho, Wo, H, W in EC.UPSAMPLE_CASES:
        assert H in (2 * Ho, 2 * Ho - 1) and W in (2 * Wo, 2 * Wo - 1)
        dy = torch.arange(2 * Ho * Wo * 4, dtype=torch.float32).view(2, Ho, Wo, 4) + 1
        o = EC.zero_upsample2_ref(dy, H, W)
        assert float(o.sum()) == float(dy.sum()) and o[1, 2 * (Ho - 1), 2 * (Wo - 1), 3] == dy[1, Ho - 1, Wo - 1, 3]
        assert H < 2 or float(o[:, 1::2].abs().sum()) == 0
        assert W < 2 or float(o[:, :, 1::2].abs().sum()) == 0


@pytest.mark.parametrize("rbn", [False, True])
@pytest.mark.parametrize("rows,C", EC.BF16_CASES[:3])
def test_bf16_tail_rule(rows, C, rbn):
    """The correct emulation passes bf16_rounded (it peaks at 1.0 against the half-ulp term alone); a thread
    holding the next channel group's scales fails it (about half of the elements fall outside)."""
    y, r, s, b, rs, rb = EC.bf16_inputs(rows, C)
    extra = (rs, rb) if rbn else ()
    ref, mag = EC.bn_add_relu_bf16_ref(y, s, b, r, *extra)
    got = EC.bn_add_relu_bf16_emulate(y, s, b, r, *extra)
    assert EC.bf16_rounded(got, ref, mag, f"emulated bn_add_relu_bf16 ({rows}, {C}) rbn={rbn}") <= 1.0
    # the bf16 -> bf16 BN + ReLU restated two ways
    x = EC.bn_relu_bf16_ref(y, s, b)
    EC.exact(x, torch.relu(torch.addcmul(b.double(), y.double(), s.double()).float()).to(EC.BF), "bn_relu_bf16 ref")
    if C > 8:
        bad = EC.bn_add_relu_bf16_emulate(y, s, b, r, *extra, group_shift=8)
        fails(EC.bf16_rounded, bad, ref, mag, "bn_add_relu_bf16 one channel group off")
        tol = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag
        assert float(((bad.double() - ref).abs() > tol).double().mean()) > 0.25
        fails(EC.exact, EC.bn_relu_bf16_ref(y, torch.roll(s, -8), torch.roll(b, -8)), x, "bn_relu_bf16 one group off")


def test_bn_eval_emulation_passes():
    for C in EC.BN_EVAL_CASES:
        gamma, beta, rm, rv = EC.bn_eval_inputs(C)
        eps = float(torch.tensor(EC.EPS, dtype=torch.float32))
        scale, shift, ms, mb = EC.bn_eval_ref(gamma, beta, rm, rv, eps)
        sc = gamma / torch.sqrt(rv + eps)
        assert EC.within(sc, scale, ms, f"fp32 bn_eval scale C={C}") < 0.5
        assert EC.within(beta - rm * sc, shift, mb, f"fp32 bn_eval shift C={C}") < 0.5
        if C > 1:  # (eps / 2 rv is up to 1e-4 of the scale among many channels)
            fails(EC.within, gamma / torch.sqrt(rv), scale, ms, "bn_eval scale without eps")
