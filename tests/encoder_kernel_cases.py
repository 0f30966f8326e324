"""Helper of the encoder non-GEMM kernel tests (not a test): the case lists, the fp64 references and the
comparison rules that tests/test_gpu_encoder_kernels.py (the kernels) and
tests/test_encoder_kernel_cases_cpu.py (the references and rules themselves) share.

Every reference takes the fp32 (or bf16) tensors that are handed to the kernel, upcasts them to fp64 and
computes there, on whatever device the tensors live. The rules:

  exact         bit equality (pure data movement, and results the arithmetic leaves exact);
  within        |got - ref| <= 4e-6 * mag + 1e-6, mag = the summed magnitudes of the element's terms
                (tests/test_gpu_gemm.py::check, the project's rule for an fp32 accumulation);
  one_rounding  |got - ref| <= 2^-24 * mag: one fp32 rounding of a value of magnitude <= mag (one fma, or
                one conversion of an fp64 value);
  bf16_rounded  |got - ref| <= 2^-8 * |ref| + 2^-22 * mag: half a bf16 ulp of the result, plus twice the
                three fp32 roundings (two fmas and one add, 2^-24 * mag each at most) before the final one.

Each returns the worst err / tol ratio and prints it; RATIOS keeps the worst per label."""
import math

import torch
import torch.nn.functional as F

RATIOS = {}
EPS = 1e-5


# ------------------------------------------------------------------------------------------ rules
def _bits(x):
    x = x.detach().contiguous()
    return x.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[x.element_size()])


def exact(got, want, what=""):
    assert got.dtype == want.dtype and got.numel() == want.numel(), f"{what}: {got.dtype} {tuple(got.shape)} " \
        f"against {want.dtype} {tuple(want.shape)}"
    a, b = _bits(got).reshape(-1).cpu(), _bits(want).reshape(-1).cpu()
    bad = a != b
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ, first at {i}: got "
                             f"{got.reshape(-1)[i].item()!r} want {want.reshape(-1)[i].item()!r}")


def _ratio(got, ref, tol, what, rule):
    got, ref = got.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    tol = tol.detach().double().reshape(-1)
    assert got.numel() == ref.numel() == tol.numel(), f"{what}: sizes {got.numel()} {ref.numel()} {tol.numel()}"
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))  # a NaN never passes
    ratio = torch.where(tol > 0, err / tol, torch.where(err > 0, torch.full_like(err, math.inf),
                                                        torch.zeros_like(err)))
    worst = float(ratio.max())
    RATIOS[what] = max(RATIOS.get(what, 0.0), worst)
    print(f"[{rule}] {what}: max err {float(err.max()):.3g}, worst err/tol ratio {worst:.3g}")
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{what} ({rule}): {int((ratio > 1).sum())}/{ratio.numel()} elements out of "
                             f"tolerance, worst err/tol ratio {worst:.3g} at {i}: got {float(got[i]):.9g} "
                             f"ref {float(ref[i]):.9g}, max err {float(err.max()):.3g}")
    return worst


def within(got, ref, mag, what):
    return _ratio(got, ref, 4e-6 * mag.double() + 1e-6, what, "within")


def one_rounding(got, ref, mag, what="one_rounding"):
    return _ratio(got, ref, 2.0 ** -24 * mag.double(), what, "one_rounding")


def bf16_rounded(got, ref, mag, what="bf16_rounded"):
    return _ratio(got, ref, 2.0 ** -8 * ref.double().abs() + 2.0 ** -22 * mag.double(), what, "bf16_rounded")


def fma32(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 (or bf16) values is exact in fp64, so this is the exact
    a*b + c rounded to fp64 and then to fp32 (equal to the single rounding but for ties of measure zero)."""
    return (a.double() * b.double() + c.double()).float()


def case_id(case):
    return "-".join(str(v) for v in case)


def _u(g, shape, scale=1.0):
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).float()


# ------------------------------------------------------------------------------------------ BN backward
# (rows, C) and the path each reaches. The slab plan is capmi_bn_bwd_reduce's host arithmetic (slab_plan
# below restates it): CB = channel float4 groups per block, RL = 256 / CB row lanes, gx channel blocks.
#   rows     C   CB   RL  gx  slabs  rows/slab  last slab   finalize trips (16 slab lanes)
#      2     4    1  256   1      1       2          2      1 (lanes 1..15 idle)
#     31     8    2  128   1      1      31         31      1; the slab is shorter than its 128 row lanes
#    545    12    3   85   1     18      31         18      2 for lanes 0 and 1; thread 255 is row lane 85,
#                                                           outside the 85-lane sum
#   8192     8    2  128   1    256      32         32      16 for every lane (CAPMI_BNB_MAX_SLABS)
#   8197     8    2  128   1    249      33         13      16 for lanes 0..8, 15 for the rest
#    100   320   64    4   2      4      25         25      1; the second channel block is a quarter full
#    392  2048   64    4   8     13      31         20      1; layer4's width
BN_CASES = [(2, 4), (31, 8), (545, 12), (8192, 8), (8197, 8), (100, 320), (392, 2048)]
BN_PLANS = {(2, 4): (1, 1, 1, 2), (31, 8): (2, 1, 1, 31), (545, 12): (3, 1, 18, 31), (8192, 8): (2, 1, 256, 32),
            (8197, 8): (2, 1, 249, 33), (100, 320): (64, 2, 4, 25), (392, 2048): (64, 8, 13, 31)}
BN_EXTRA_CASES = [(545, 12), (392, 2048)]  # accumulate, determinism, in-place and tail forms
BN_APPLY_BIG = (8193, 2048)                # rows * C / 4 > 16384 * 256: the apply's grid-stride loop
BNB_MAX_SLABS = 256
BNB_FIN_LANES = 16


def slab_plan(rows, C):
    """(CB, gx, slabs, rows per slab) of capmi_bn_bwd_reduce (csrc/encoder_bwd.hip)."""
    C4 = C // 4
    CB = min(64, C4)
    gx = (C4 + CB - 1) // CB
    slabs = min(BNB_MAX_SLABS, max(1, 2048 // gx))
    slabs = min(slabs, (rows + 31) // 32)
    per = (rows + slabs - 1) // slabs
    return CB, gx, (rows + per - 1) // per, per


def bn_inputs(rows, C, seed=None):
    """fp32 inputs of one BN backward, as the fine-tune backward hands them over: the pre-BN conv output y,
    the upstream gradient d, gamma / beta, the batch mean and (biased) variance rounded to fp32 as
    bn_finalize saves them, the forward's fp32 scale / shift (mode 0's mask) and the saved block output
    out = relu(fma(y, scale, shift) + res) (mode 1's mask).

    rows = 2 is special: BN backward of two samples is dy = k1 (dz1 - dz2) / 2 * eps / (var + eps) (x^ is +-
    sqrt(var / (var + eps))), a cancellation by eps / var that no fp32 kernel survives unless var <~ eps. So
    that case draws y on a 2^-12 grid within 2^-9 of a per-channel centre on a 2^-4 grid: var <= 2^-18 < eps,
    and mean and var are exact in fp32."""
    g = torch.Generator().manual_seed(7919 * rows + C if seed is None else seed)
    if rows == 2:
        centre = torch.randint(-16, 17, (1, C), generator=g).float() / 16
        y = centre + torch.randint(-8, 9, (rows, C), generator=g).float() / 4096
    else:
        y = _u(g, (rows, C), 2.0) + 0.3
    gamma, beta = _u(g, (C,)) + 1.0, _u(g, (C,), 0.3)
    d, res = _u(g, (rows, C)), _u(g, (rows, C))
    y64 = y.double()
    mean = y64.mean(0).float()
    var = y64.var(0, unbiased=False).float()
    eps = float(torch.tensor(EPS, dtype=torch.float32))  # the entry point takes eps as a float
    inv = 1.0 / torch.sqrt(var.double() + eps)
    scale = (gamma.double() * inv).float()
    shift = (beta.double() - mean.double() * scale.double()).float()
    out = torch.relu(fma32(y, scale, shift) + res)
    return dict(rows=rows, C=C, eps=eps, y=y, d=d, gamma=gamma, beta=beta, mean=mean, var=var, scale=scale,
                shift=shift, out=out)


def bn_mask(mode, p):
    """The forward's ReLU branch, exactly: mode 0 the sign of y * scale + shift (the product is exact in
    fp64 and the rounded sum keeps the exact sum's sign, which is also the sign of the kernel's fp32 fma);
    mode 1 [out > 0] of the saved output."""
    if mode == 0:
        return p["y"].double() * p["scale"].double() + p["shift"].double() > 0
    return p["out"] > 0


def bn_dz(mode, p):
    """dz = d where the ReLU passed, +0 elsewhere (as the kernel selects it: no -0 from a product), fp64."""
    d = p["d"].double()
    return torch.where(bn_mask(mode, p), d, torch.zeros_like(d))


def bn_bwd_ref(mode, p):
    """fp64 closed form of BatchNorm2d(train) (+ReLU) backward from the kernel's own fp32 inputs. Returns
    dz, dbeta, dgamma, coef (4, C) = [k1, k1 invstd dgamma / n, k1 dbeta / n, mean], dy and the magnitudes
    (sums of the absolute terms) that go with them."""
    n = p["rows"]
    mask = bn_mask(mode, p)
    dz = bn_dz(mode, p)
    xc = p["y"].double() - p["mean"].double()
    inv = 1.0 / torch.sqrt(p["var"].double() + p["eps"])
    dbeta, mag_db = dz.sum(0), dz.abs().sum(0)
    dgamma, mag_dg = inv * (dz * xc).sum(0), inv * (dz.abs() * xc.abs()).sum(0)
    k1 = p["gamma"].double() * inv
    coef = torch.stack([k1, k1 * inv * dgamma / n, k1 * dbeta / n, p["mean"].double()])
    mag_coef = torch.stack([k1.abs(), k1.abs() * inv * mag_dg / n, k1.abs() * mag_db / n, p["mean"].double().abs()])
    dy = k1 * dz - coef[1] * xc - coef[2]
    return dict(mask=mask, dz=dz, xc=xc, dbeta=dbeta, dgamma=dgamma, mag_db=mag_db, mag_dg=mag_dg, coef=coef,
                mag_coef=mag_coef, dy=dy)


def bn_apply_ref(dz, y, coef):
    """dy = coef0 dz - coef1 (y - coef3) - coef2 in fp64 from a given fp32 coef (4C, or (4, C)), and its
    magnitude |coef0||dz| + |coef1||y - coef3| + |coef2|."""
    c = coef.double().view(4, -1)
    xc = y.double() - c[3]
    return c[0] * dz - c[1] * xc - c[2], c[0].abs() * dz.abs() + c[1].abs() * xc.abs() + c[2].abs()


def bn_bwd_autograd(p, dz):
    """fp64 autograd through F.batch_norm(training=True) on the fp32 y, fed dz: (dy, dgamma, dbeta)."""
    y = p["y"].double().t().unsqueeze(0).clone().requires_grad_()  # (1, C, rows)
    g, b = p["gamma"].double().clone().requires_grad_(), p["beta"].double().clone().requires_grad_()
    F.batch_norm(y, None, None, g, b, training=True, eps=p["eps"]).backward(dz.double().t().unsqueeze(0))
    return y.grad[0].t(), g.grad, b.grad


def bn_bwd_emulate(mode, p, drop_last_slab=False, max_slabs=None):
    """fp32 CPU emulation of the two-stage sum: per-slab fp32 partials (plain fp32 sums of dz and of
    dz * (y - mean)), an fp64 total over the slabs, the finalize's fp64 algebra rounded to fp32. The two
    options emulate plausible bugs: the last (partial) slab never summed; only slabs 0..max_slabs-1 summed
    (the finalize lanes' first trip alone is max_slabs = 16). Returns fp32 dgamma, dbeta, coef (4C)."""
    rows, C = p["rows"], p["C"]
    _, _, slabs, per = slab_plan(rows, C)
    dz = p["d"] * bn_mask(mode, p)
    xc = p["y"] - p["mean"]
    s, q = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    last = slabs - 1 if drop_last_slab else slabs
    if max_slabs is not None:
        last = min(last, max_slabs)
    for k in range(last):
        r0, r1 = k * per, min(rows, (k + 1) * per)
        s += dz[r0:r1].sum(0).double()
        q += (dz[r0:r1] * xc[r0:r1]).sum(0).double()
    inv = 1.0 / torch.sqrt(p["var"].double() + p["eps"])
    dg, db = q * inv, s
    k1 = p["gamma"].double() * inv
    coef = torch.stack([k1, k1 * inv * dg / rows, k1 * db / rows, p["mean"].double()]).float().reshape(-1)
    return dg.float(), db.float(), coef


def check_bn_reduce(dgamma, dbeta, coef, p, ref, what):
    """The reduce's outputs against the fp64 closed form; returns the worst ratios by output."""
    C = p["C"]
    c = coef.reshape(4, C)
    r = {"dgamma": within(dgamma, ref["dgamma"], ref["mag_dg"], f"{what} dgamma"),
         "dbeta": within(dbeta, ref["dbeta"], ref["mag_db"], f"{what} dbeta"),
         "coef0": one_rounding(c[0], ref["coef"][0], ref["mag_coef"][0], f"{what} coef0"),
         "coef1": within(c[1], ref["coef"][1], ref["mag_coef"][1], f"{what} coef1"),
         "coef2": within(c[2], ref["coef"][2], ref["mag_coef"][2], f"{what} coef2")}
    exact(c[3], p["mean"].to(c.device), f"{what} coef3")
    return r


# ------------------------------------------------------------------------------------------ conv1 tail
# (N, H, W, C): odd sizes with H != W; a single-pixel window; H = 2; the production map; past the
# 8192-block grid (2 * 258 * 258 * 16 float4 > 8192 * 256) with odd sizes
MAXPOOL_CASES = [(2, 9, 7, 8), (1, 1, 1, 4), (1, 2, 5, 4), (3, 112, 112, 64), (2, 515, 515, 64)]


def maxpool_out(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def maxpool_inputs(N, H, W, C):
    """y (N, H, W, C), scale, shift; the last channel's shift is below -max|y * scale|, so relu leaves only
    zeros there: the answer is a window of zeros, never the -inf the running maximum starts from."""
    g = torch.Generator().manual_seed(31 * N + 7 * H + 3 * W + C)
    y = _u(g, (N, H, W, C), 2.0)
    s, b = _u(g, (C,)) + 1.25, _u(g, (C,), 0.5)
    b[C - 1] = -6.0
    return y, s, b


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def maxpool_ref(y, s, b):
    """fp64 F.max_pool2d(relu(y * s + b), 3, 2, 1) in NHWC and the magnitude: the window maximum of
    |y||s| + |b| (relu and max round nothing; the selected element's own magnitude is at most that)."""
    v = y.double() * s.double() + b.double()
    ref = F.max_pool2d(_nchw(torch.relu(v)), 3, 2, 1)
    mag = F.max_pool2d(_nchw(y.double().abs() * s.double().abs() + b.double().abs()), 3, 2, 1)
    return _nhwc(ref), _nhwc(mag)


def maxpool_emulate(y, s, b, skip_row_past_end=True):
    """fp32 CPU emulation: fma, relu, 3x3/2 window maximum. skip_row_past_end=False is the bug of a window
    row ih = H not being skipped: it reads the next image's first row (the row after the last image's end
    is taken from the first image: whatever lies there)."""
    N, H, W, C = y.shape
    v = torch.relu(fma32(y, s, b))
    below = torch.roll(v[:, :1], -1, 0) if not skip_row_past_end else torch.full_like(v[:, :1], -math.inf)
    v = torch.cat([v, below], 1)  # row H
    v = F.pad(_nchw(v), (1, 1, 1, 0), value=-math.inf)  # left, right, top
    return _nhwc(F.max_pool2d(v, 3, 2, 0))


# ------------------------------------------------------------------------------------------ pools
# (N, H, W, OH, OW, C), shared by adaptive_avgpool_nhwc, its backward and adaptive_avgpool_bf16
POOL_CASES = [(2, 7, 7, 14, 14, 2048),   # the production replicate: forward bit-equal to the gathered input
              (2, 7, 5, 14, 10, 8),
              (2, 5, 9, 3, 4, 8),
              (2, 9, 9, 4, 4, 8),
              (2, 3, 3, 1, 1, 8),
              (2, 1, 1, 2, 3, 8),
              (2, 14, 14, 14, 14, 8),    # identity: bit-equal
              (48, 7, 7, 14, 14, 2048)]  # 48 * 196 * 512 float4 > 8192 * 256: the forward's grid-stride loop
POOL_GATHER_CASES = [c for c in POOL_CASES if c[3] % c[1] == 0 and c[4] % c[2] == 0]  # every window one pixel


def pool_inputs(N, H, W, OH, OW, C, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 * H + 100 * W + 10 * OH + OW + N + C)
    return _u(g, (N, H, W, C)).to(dtype), _u(g, (N, OH, OW, C))


def pool_fwd_ref(x, OH, OW):
    """fp64 F.adaptive_avg_pool2d of an NHWC map and its magnitude (the pooled |x|)."""
    x = _nchw(x.double())
    return _nhwc(F.adaptive_avg_pool2d(x, (OH, OW))), _nhwc(F.adaptive_avg_pool2d(x.abs(), (OH, OW)))


def pool_gather(x, OH, OW):
    """The replicate form (OH, OW multiples of H, W): every output cell is one input pixel."""
    N, H, W, C = x.shape
    ih = torch.arange(OH, device=x.device) * H // OH
    iw = torch.arange(OW, device=x.device) * W // OW
    return x[:, ih][:, :, iw].contiguous()


def pool_bwd_ref(d, H, W):
    """fp64 autograd of F.adaptive_avg_pool2d for the NHWC output gradient d, and the same of |d|."""
    N, OH, OW, C = d.shape
    x = torch.zeros(N, C, H, W, dtype=torch.float64, device=d.device, requires_grad=True)
    out = F.adaptive_avg_pool2d(x, (OH, OW))
    g, = torch.autograd.grad(out, x, _nchw(d.double()), retain_graph=True)
    m, = torch.autograd.grad(out, x, _nchw(d.double().abs()))
    return _nhwc(g), _nhwc(m)


def pool_fwd_swapped(x, OH, OW):
    """The bug of H and W (and OH and OW) swapped in the index arithmetic: the same buffers walked as
    (N, W, H, C) -> (N, OW, OH, C). fp32."""
    N, H, W, C = x.shape
    o = F.adaptive_avg_pool2d(_nchw(x.float().reshape(N, W, H, C)), (OW, OH))
    return _nhwc(o).reshape(N, OH, OW, C)


def pool_bwd_swapped(d, H, W):
    N, OH, OW, C = d.shape
    g, _ = pool_bwd_ref(d.reshape(N, OW, OH, C), W, H)
    return g.float().reshape(N, H, W, C)


# ------------------------------------------------------------------------------------------ layouts
# (Cout, Cin, KH, KW, Cin_pad): conv1; KH != KW both ways (with a 1 x 3 or 3 x 1 kernel [kh][kw] and [kw][kh] are
# the same buffer, so these show a wrong extent or flip, not a swap); 2 x 3, where a swap shows; 2.36 M elements,
# past the 8192-block grid
PACK_CASES = [(64, 3, 7, 7, 4), (5, 3, 1, 3, 8), (7, 6, 3, 1, 6), (6, 5, 2, 3, 8), (512, 512, 3, 3, 512)]
PACK_S2_CASES = [(5, 3), (128, 64)]  # (Cout, Cin), every parity class (ph, pw)
IMAGE_CASES = [(2, 1, 5, 7), (2, 3, 6, 5), (3, 4, 3, 9), (0, 3, 4, 6)]  # (N, C, H, W)
UPSAMPLE_CASES = [(3, 4, 6, 8), (3, 4, 5, 7), (1, 1, 1, 1)]  # (Ho, Wo, H, W): H = 2 Ho, 2 Ho - 1
BN_EVAL_CASES = [1, 257, 2048]


def weights(Cout, Cin, KH, KW):
    g = torch.Generator().manual_seed(Cout * 1000 + Cin * 100 + KH * 10 + KW)
    return _u(g, (Cout, Cin, KH, KW))


def pack_pad_ref(w, cin_pad):
    """out[co][kh][kw][cp] = w[co][cp][kh][kw], zero for cp >= Cin."""
    co, ci, kh, kw = w.shape
    out = torch.zeros(co, kh, kw, cin_pad, dtype=w.dtype, device=w.device)
    out[..., :ci] = w.permute(0, 2, 3, 1)
    return out


def pack_pad_khkw_swapped(w, cin_pad):
    """The bug of kh and kw swapped in the output index: the buffer written as [co][kw][kh][cp]."""
    co, ci, kh, kw = w.shape
    out = torch.zeros(co, kw, kh, cin_pad, dtype=w.dtype)
    out[..., :ci] = w.permute(0, 3, 2, 1)
    return out


def pack_dgrad_ref(w):
    """out[ci][kh][kw][co] = w[co][ci][KH-1-kh][KW-1-kw]"""
    return w.flip(2, 3).permute(1, 2, 3, 0).contiguous()


def pack_dgrad_khkw_swapped(w):
    return w.flip(2, 3).permute(1, 3, 2, 0).contiguous()


def unpack_ref(packed, shape):
    """[Cout][KH][KW][Cin] -> [Cout][Cin][KH][KW]"""
    co, ci, kh, kw = shape
    return packed.reshape(co, kh, kw, ci).permute(0, 3, 1, 2).contiguous()


def unpack_khkw_swapped(packed, shape):
    co, ci, kh, kw = shape
    return packed.reshape(co, kw, kh, ci).permute(0, 3, 2, 1).contiguous()


def pack_dgrad_s2_ref(w, ph, pw):
    """out[ci][th][tw][co] = w[co][ci][kh(th)][kw(tw)], kh = 1 if ph == 0 else 2 - 2 th (same along w)."""
    khs = [1] if ph == 0 else [2 - 2 * th for th in range(2)]
    kws = [1] if pw == 0 else [2 - 2 * tw for tw in range(2)]
    return w[:, :, khs][:, :, :, kws].permute(1, 2, 3, 0).contiguous()


def image_nhwc4_ref(imgs):
    N, C, H, W = imgs.shape
    out = torch.zeros(N, H, W, 4, dtype=imgs.dtype, device=imgs.device)
    out[..., :C] = imgs.permute(0, 2, 3, 1)
    return out


def zero_upsample2_ref(dy, H, W):
    N, Ho, Wo, C = dy.shape
    out = torch.zeros(N, H, W, C, dtype=dy.dtype, device=dy.device)
    out[:, 0:2 * Ho:2, 0:2 * Wo:2] = dy
    return out


def bn_eval_inputs(C):
    g = torch.Generator().manual_seed(4000 + C)
    return _u(g, (C,)) + 1.0, _u(g, (C,), 0.5), _u(g, (C,)), torch.rand(C, generator=g) + 0.05


def bn_eval_ref(gamma, beta, rm, rv, eps):
    """fp64 scale = gamma / sqrt(rv + eps), shift = beta - rm * scale and their magnitudes."""
    scale = gamma.double() / torch.sqrt(rv.double() + eps)
    return (scale, beta.double() - rm.double() * scale, scale.abs(),
            beta.double().abs() + rm.double().abs() * scale.abs())


# ------------------------------------------------------------------------------------------ bf16 BN kernels
# (rows, C): one chunk; C/8 = 8; C/8 = 256 (a block is one row); n8 = 1 048 600 > 4096 * 256 threads, so
# threads 0..23 take a second trip of the grid-stride loop and must land on their channel group again
BF16_CASES = [(1, 8), (1000, 64), (777, 2048), (131075, 64)]
BF = torch.bfloat16


def bf16_inputs(rows, C):
    """bf16 y and residual; per-channel fp32 scales / shifts whose size depends on the channel, so a wrong
    channel group is far outside any rounding."""
    g = torch.Generator().manual_seed(rows * 13 + C)
    y, r = _u(g, (rows, C), 3.0).to(BF), _u(g, (rows, C), 3.0).to(BF)
    s, b = torch.rand(C, generator=g) * 1.5 + 0.5, torch.rand(C, generator=g) * 2 - 0.5
    rs, rb = torch.rand(C, generator=g) * 1.5 + 0.5, torch.rand(C, generator=g) * 2 - 1
    return y, r, s, b, rs, rb


def bn_relu_bf16_ref(y, s, b):
    """relu(fma(y, s, b)) rounded to bf16 once (RNE): the kernel bit for bit."""
    return torch.relu(fma32(y, s, b)).to(BF)


def bn_add_relu_bf16_ref(y, s, b, r, rs=None, rb=None):
    """fp64 relu(y s + b + r') with r' = r or r rs + rb, and the magnitude of its terms."""
    yd, rd = y.double(), r.double()
    v, mag = yd * s.double() + b.double(), yd.abs() * s.double().abs() + b.double().abs()
    if rs is not None:
        v, mag = v + rd * rs.double() + rb.double(), mag + rd.abs() * rs.double().abs() + rb.double().abs()
    else:
        v, mag = v + rd, mag + rd.abs()
    return torch.relu(v), mag


def bn_add_relu_bf16_emulate(y, s, b, r, rs=None, rb=None, group_shift=0):
    """fp32 CPU emulation of the kernel: two fmas, one add, relu, one RNE rounding to bf16. group_shift = 8 is
    the bug of a thread holding the scales / shifts of the next channel group."""
    if group_shift:
        s, b = torch.roll(s, -group_shift), torch.roll(b, -group_shift)
        if rs is not None:
            rs, rb = torch.roll(rs, -group_shift), torch.roll(rb, -group_shift)
    rr = r.float() if rs is None else fma32(r, rs, rb)
    return torch.relu(fma32(y, s, b) + rr).to(BF)
