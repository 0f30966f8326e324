"""Helper of the GEMM contract tests (not a test): the case table, the inputs and the fp64 restatement of the
epilogue and addressing contract of include/capmi.h,

    C = alpha * alpha_ptr[0] * op(A).op(B) (+ bias + bias2) (+ beta*C) (relu)

stored through ldc and the c_r1 / c_s2 row remap, which tests/test_gpu_gemm_contract.py runs every GEMM kernel
form against and tests/test_gemm_contract_cases_cpu.py checks on the CPU (against torch built independently, the
cases' own preconditions, and the launch sites of csrc/gemm_nt.hip).

A case is one launch: a kernel family, the API it goes through (``gemm``: capmi_gemm / capmi_gemm_ex, the
data-parallel grids; ``sk``: capmi_gemm_sk_ex), operand modes, tile, flags, the problem geometry and one of the
epilogue configurations

  plain        alpha 1, no bias, beta 0, no relu, no remap: C is a column sub-view (ldc = N + 12) prefilled with
               NaN inside the view and a canary everywhere else (padding columns, a guard row above, 8 rows
               below M); statistics where the family takes them;
  plain_beta1  the same with beta 1 onto a finite C0 (the x3 kernels' store-only epilogue with the C load);
  full         alpha -0.75, alpha_ptr -> 1.5, bias and bias2, beta 0.5 onto a finite C0, relu, ldc > N, and the
               A / C row remaps and statistics where the form takes them (``fields`` narrows it to what the
               header documents for gemm_x3w: alpha / beta only).

Each case names the kernel instantiation it must launch (``expect``, what capmi_last_launch_name returns).

Data-parallel forms that a small problem cannot reach through capmi_gemm_ex: a problem with the BN prologue is
sent to the fp32 kernel there, so the prologue arms of the split-staged and bf16 kernels are run data-parallel
through capmi_gemm_sk_ex with ksplit = 2 (a k-split is never stream-K): two raw partial slabs, each pinned to
its own k range, the bias in slab 0 only. UNREACHABLE lists the launch sites no host path reaches at all."""
import math
import re
from dataclasses import dataclass
from types import SimpleNamespace

import torch

F64 = torch.float64
CANARY = -1234.5677490234375          # exact in fp32; never a result of these problems
EINVAL = 1001
TILE_128, TILE_64, TILE_128x64, TILE_AUTO, TILE_W8 = 0, 1, 2, 3, 4
BF16, X3, X3P, SPLIT3, X3D, X3S, X3W, X3C = 1, 4, 8, 16, 32, 64, 128, 256
TILE_DIMS = {TILE_64: (64, 64), TILE_128x64: (128, 64), TILE_128: (128, 128)}
ALPHA, ALPHA_PTR, BETA = -0.75, 1.5, 0.5
R1 = 5                                # rows per group of the 2-level row remaps
GUARD_ROWS = 8                        # canary rows below M
SLAB_GAP = 16                         # canary floats between k-split slabs
BF16_FAMILIES = ("nts1", "bf16", "w16")
RATIOS = {}


@dataclass(frozen=True)
class Case:
    id: str
    family: str
    api: str            # "gemm" | "sk"
    amode: int
    bmode: int
    tile: int
    flags: int
    cfg: str            # "plain" | "plain_beta1" | "full"
    geoms: tuple        # one geometry per problem of the launch
    expect: str
    sk: bool = False    # stream-K expected
    pro: bool = False
    stats: bool = False
    a_remap: bool = False
    c_remap: bool = False
    ksplits: tuple = (1,)
    ws: bool = True     # pass the stream-K workspace (api "sk")
    fields: str = "all"  # "all" | "alpha_beta" (gemm_x3w's documented contract) | "bias" (plain plus a bias:
    #                      the grouped k-split launches, whose slabs are raw partials)
    unaligned: bool = False  # odd leading dimensions: the generic kernel's scalar loads
    refuse: str = ""    # "" | the field the family's contract omits: the launch must return EINVAL


def b(v):
    return "true" if v else "false"


# ------------------------------------------------------------------------------------------ geometry
def dims(geom):
    """(M, N, K, conv geometry or None) of one problem."""
    kind = geom[0]
    if kind == "dense":
        return geom[1], geom[2], geom[3], None
    if kind == "conv1":
        n, H, W, Cout = geom[1:]
        geom = ("conv", n, H, W, 4, 7, 2, 3, Cout)
        kind = "conv"
    n, H, W, Cin, k, s, p, Cout = geom[1:]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    geo = dict(N=n, H=H, W=W, Cin=Cin, KH=k, KW=k, stride=s, pad=p, Ho=Ho, Wo=Wo)
    if kind == "conv":
        return n * Ho * Wo, Cout, k * k * Cin, geo
    assert kind == "wgrad", kind
    return Cout, k * k * Cin, n * Ho * Wo, geo


def remap(r, r1, ld, s2):
    """The 2-level row remap of capmi_gemm_problem: off(r) = (r % r1)*ld + (r / r1)*s2, or r*ld."""
    return (r % r1) * ld + (r // r1) * s2 if r1 > 0 else r * ld


def layout(case, i=0):
    """Every size, stride and offset of problem i of a case (no data)."""
    L = SimpleNamespace()
    L.M, L.N, L.K, L.geo = dims(case.geoms[i])
    M, N, K = L.M, L.N, L.K
    fam = case.family
    x3fam = fam in ("x3", "x3p", "x3d", "x3s", "x3c")
    odd = 1 if case.unaligned else 0
    # ---- A
    L.a_r1 = L.a_s2 = 0
    if case.amode == 0:
        pad = 8 if fam == "x3p" else 0 if (fam == "x3d" and case.pro) else 1 if odd else 4
        L.a_width, L.a_rows = K + pad, M
        L.lda = L.a_width
        if case.a_remap:
            t2 = -(-M // R1)
            L.a_rows, L.lda, L.a_r1, L.a_s2 = R1 * t2, t2 * L.a_width, R1, L.a_width
        L.a_shape = (L.a_rows, L.a_width)
    elif case.amode == 1:
        L.a_width, L.a_rows = M + 4, K
        L.lda = L.a_width
        if case.a_remap:
            t2 = -(-K // R1)
            L.a_rows, L.lda, L.a_r1, L.a_s2 = R1 * t2, t2 * L.a_width, R1, L.a_width
        L.a_shape = (L.a_rows, L.a_width)
    else:
        g = L.geo
        L.lda = 0
        L.a_shape = (g["N"], g["Cin"], g["H"], g["W"]) if case.amode == 3 else (g["N"], g["H"], g["W"], g["Cin"])
    # ---- B
    if case.bmode == 0:
        pad = 0 if fam == "x3c" else 8 if x3fam else 1 if odd else 4
        L.ldb = K + pad
        L.b_shape = (N, L.ldb)
    elif case.bmode == 1:
        L.ldb = N + 4
        L.b_shape = (K, L.ldb)
    else:
        g = L.geo
        L.ldb = 0
        L.b_shape = (g["N"], g["H"], g["W"], g["Cin"])
    # ---- C: a column sub-view of rows of width N + 12, a guard row above, GUARD_ROWS below
    assert N % 4 == 0
    L.c_width = N + 12
    L.c_off = L.c_width + 4
    L.c_r1 = L.c_s2 = 0
    L.ldc = L.c_width
    L.c_rows = M
    if case.c_remap:
        t2 = -(-M // R1)
        L.c_rows, L.ldc, L.c_r1, L.c_s2 = R1 * t2, t2 * L.c_width, R1, L.c_width
    L.ksplit = case.ksplits[i]
    L.c_split_stride = (L.c_rows + GUARD_ROWS) * L.c_width + SLAB_GAP if L.ksplit > 1 else 0
    slab = (L.c_rows + GUARD_ROWS) * L.c_width + SLAB_GAP
    L.c_numel = L.c_off + L.ksplit * slab
    # k range of slab z (plan_nt_group, csrc/gemm_plan.hip: the chunk rounded up to the v2 kernel's k-tile of 32)
    kc = -(-K // L.ksplit)
    kc = -(-kc // 32) * 32
    L.k_ranges = [(min(K, z * kc), min(K, (z + 1) * kc)) for z in range(L.ksplit)]
    L.stat_slices = -(-M // 64)
    return L


def c_offsets(L):
    """Offsets into the C buffer of logical element (slab z, row r, column c): [ksplit, M, N] int64."""
    r = torch.arange(L.M)
    row = torch.tensor([remap(int(x), L.c_r1, L.ldc, L.c_s2) for x in r], dtype=torch.int64)
    off = L.c_off + row[:, None] + torch.arange(L.N)[None, :]
    return torch.stack([off + z * L.c_split_stride for z in range(L.ksplit)])


# ------------------------------------------------------------------------------------------ epilogue fields
def epilogue(case):
    """(alpha, alpha_ptr or None, beta, relu, bias?, bias2?) of a case's configuration."""
    if case.refuse:
        f = case.refuse
        return (ALPHA if f == "alpha" else 1.0, None, BETA if f == "beta" else 0.0, f == "relu", f == "bias", False)
    if case.cfg == "plain":
        return 1.0, None, 0.0, False, case.fields == "bias", False
    if case.cfg == "plain_beta1":
        return 1.0, None, 1.0, False, False, False
    if case.fields == "alpha_beta":
        return ALPHA, ALPHA_PTR, BETA, False, False, False
    return ALPHA, ALPHA_PTR, BETA, True, True, True


# ------------------------------------------------------------------------------------------ the restatement
def _bf(x):
    return x.to(torch.bfloat16).to(F64)


def _prologue(x, sc, sh, bf16):
    """relu(x*scale[ci] + shift[ci]) on the channel axis (last); the bf16 forms run it in fp32 (one fma)
    before they round the operand."""
    v = x.double() * sc.double() + sh.double()
    if bf16:
        v = v.float().double()
    return torch.relu(v)


def _im2col(x, geo):
    """x [n, H, W, C] (fp64, prologue applied) -> [n*Ho*Wo, KH, KW, C]; a tap outside the image is zero."""
    n, H, W, C = x.shape
    s, p = geo["stride"], geo["pad"]
    ih = torch.arange(geo["Ho"])[:, None] * s - p + torch.arange(geo["KH"])[None, :]
    iw = torch.arange(geo["Wo"])[:, None] * s - p + torch.arange(geo["KW"])[None, :]
    okh, okw = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
    g = x[:, ih.clamp(0, H - 1)]                      # [n, Ho, KH, W, C]
    g = g[:, :, :, iw.clamp(0, W - 1)]                # [n, Ho, KH, Wo, KW, C]
    g = g * (okh[:, :, None, None] & okw[None, None, :, :])[None, :, :, :, :, None]
    return g.permute(0, 1, 3, 2, 4, 5).reshape(n * geo["Ho"] * geo["Wo"], geo["KH"], geo["KW"], C)


def operands(case, L, p):
    """The logical operands op(A) [M, K] and op(B) [K, N] in fp64, as the kernel's mode reads them."""
    bf16 = case.family in BF16_FAMILIES
    A, B = p["A"], p["B"]
    if case.amode == 0:
        idx = torch.tensor([remap(r, L.a_r1, L.lda, L.a_s2) for r in range(L.M)], dtype=torch.int64)
        Al = A.reshape(-1)[idx[:, None] + torch.arange(L.K)[None, :]].double()
        if case.pro:  # x3d: dense rows of a 1x1 conv's input, k is the channel
            Al = _prologue(Al, p["in_scale"], p["in_shift"], bf16)
    elif case.amode == 1:
        idx = torch.tensor([remap(k, L.a_r1, L.lda, L.a_s2) for k in range(L.K)], dtype=torch.int64)
        Al = A.reshape(-1)[idx[:, None] + torch.arange(L.M)[None, :]].double().T
    else:
        x = A.permute(0, 2, 3, 1) if case.amode == 3 else A
        x = _prologue(x, p["in_scale"], p["in_shift"], bf16) if case.pro else x.double()
        col = _im2col(x, L.geo)                       # k = (kh, kw, ci)
        if case.amode == 3:
            col = col.permute(0, 3, 1, 2)             # k = (ci, kh, kw)
        Al = col.reshape(L.M, L.K)
    if case.bmode == 0:
        Bl = B[:, :L.K].double().T
    elif case.bmode == 1:
        Bl = B[:, :L.N].double()
    else:
        x = _prologue(B, p["in_scale"], p["in_shift"], bf16) if case.pro else B.double()
        Bl = _im2col(x, L.geo).reshape(L.K, L.N)      # k = output pixel, n = (kh, kw, ci)
    if bf16:
        Al, Bl = _bf(Al), _bf(Bl)
    return Al, Bl


def gemm_contract_ref(case, inp):
    """Per problem: (expected, bound), each [ksplit, M, N] fp64, of the values stored at c_offsets(layout).
    bound = |alpha*alpha_ptr| (|A|.|B|) + |bias| + |bias2| + |beta| |C0|."""
    alpha, aptr, beta, relu, _, _ = epilogue(case)
    eff = float(torch.tensor(alpha, dtype=torch.float32) * torch.tensor(1.0 if aptr is None else aptr,
                                                                        dtype=torch.float32))
    out = []
    for i, p in enumerate(inp):
        L = layout(case, i)
        Al, Bl = operands(case, L, p)
        offs = c_offsets(L)
        exp, bnd = [], []
        for z, (k0, k1) in enumerate(L.k_ranges):
            v = eff * (Al[:, k0:k1] @ Bl[k0:k1])
            m = abs(eff) * (Al[:, k0:k1].abs() @ Bl[k0:k1].abs())
            if z == 0:
                for name in ("bias", "bias2"):
                    if p.get(name) is not None:
                        v = v + p[name].double()[None, :]
                        m = m + p[name].double().abs()[None, :]
            if beta != 0.0:
                c0 = p["C"].reshape(-1)[offs[z]].double()
                v = v + beta * c0
                m = m + abs(beta) * c0.abs()
            if relu:
                v = torch.relu(v)
            exp.append(v)
            bnd.append(m)
        out.append((torch.stack(exp), torch.stack(bnd)))
    return out


# ------------------------------------------------------------------------------------------ inputs
def _u(g, shape, scale=1.0):
    return ((torch.rand(shape, generator=g, dtype=F64) * 2 - 1) * scale).float()


def make_inputs(case):
    """The fp32 CPU tensors of a case, one dict per problem, in the layout handed to the kernel: A, B, C (the
    whole buffer: canaries, and NaN or C0 in the view), bias, bias2, alpha_ptr, in_scale, in_shift, stats."""
    seed = int.from_bytes(case.id.encode(), "little") % (2 ** 31 - 1)
    g = torch.Generator().manual_seed(seed)
    alpha, aptr, beta, relu, has_b1, has_b2 = epilogue(case)
    out = []
    for i in range(len(case.geoms)):
        L = layout(case, i)
        p = {"A": _u(g, L.a_shape), "B": _u(g, L.b_shape)}
        if i > 0:
            p["A"] = out[0]["A"]  # grouped problems share A (the decoder's per-timestep form)
        p["bias"] = _u(g, (L.N,)) if has_b1 else None
        p["bias2"] = _u(g, (L.N,)) if has_b2 else None
        p["alpha_ptr"] = torch.tensor([aptr], dtype=torch.float32) if aptr is not None else None
        cin = L.geo["Cin"] if L.geo else L.K
        p["in_scale"] = _u(g, (cin,), 1.5) if case.pro else None
        p["in_shift"] = _u(g, (cin,), 0.5) if case.pro else None
        C = torch.full((L.c_numel,), CANARY, dtype=torch.float32)
        offs = c_offsets(L)
        if beta == 0.0:
            C[offs.reshape(-1)] = float("nan")
        else:
            # C0 of the product's own size: rms(beta*C0) == rms(alpha*alpha_ptr*A.B)
            Al, Bl = operands(case, L, p)
            rms = float((Al @ Bl).pow(2).mean().sqrt()) * abs(alpha * (aptr or 1.0))
            C[offs.reshape(-1)] = _u(g, (offs.numel(),), math.sqrt(3.0) * rms / abs(beta))
        p["C"] = C
        p["stats"] = torch.full((L.stat_slices + 2, L.N, 2), CANARY, dtype=torch.float32) if case.stats else None
        out.append(p)
    return out


def c_view_mask(case, i=0):
    """bool [c_numel]: the elements of the C buffer the launch may write."""
    L = layout(case, i)
    m = torch.zeros(L.c_numel, dtype=torch.bool)
    m[c_offsets(L).reshape(-1)] = True
    return m


# ------------------------------------------------------------------------------------------ comparison rules
def ratio(got, ref, tol):
    err = (got.double() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))  # a NaN never passes
    return float((err / tol).max()) if err.numel() else 0.0


def check_result(case, got, ref, bound):
    """|C - ref| <= 4e-6 * bound + 1e-6 (tests/test_gpu_gemm.py's rule with the epilogue's terms in the bound;
    the bf16-operand forms against the reference of the rounded operands). Returns the worst err / tol."""
    worst = ratio(got, ref, 4e-6 * bound + 1e-6)
    RATIOS[case.family] = max(RATIOS.get(case.family, 0.0), worst)
    print(f"[{case.family}] {case.id}: worst err/tol {worst:.3g}")
    assert worst <= 1.0, f"{case.id}: result outside 4e-6*bound + 1e-6, worst err/tol {worst:.3g}"
    return worst


def check_stats(case, L, stored, stats):
    """stats[slice][col] against the fp64 sums of the kernel's own stored C over the slice's 64 rows:
    2 * 64 * 2^-24 * sum|v| (sum v^2) + 1e-6, the bound of a 64-term fp32 sum in any grouping. Slices past
    ceil(M/64) keep their canary."""
    st = stats.double()
    v = stored.double()
    u = 2 * 64 * 2.0 ** -24
    for s in range(L.stat_slices):
        rows = v[64 * s: 64 * (s + 1)]
        for j, (want, mag) in enumerate(((rows.sum(0), rows.abs().sum(0)), ((rows * rows).sum(0),) * 2)):
            r = ratio(st[s, :, j], want, u * mag + 1e-6)
            assert r <= 1.0, f"{case.id}: stats slice {s} {'sum' if j == 0 else 'sumsq'} off, err/tol {r:.3g}"
    tail = stats[L.stat_slices:]
    assert bool((tail.view(torch.int32) == torch.tensor(CANARY).view(torch.int32)).all()), \
        f"{case.id}: statistics written past slice {L.stat_slices - 1}"


def check_canaries(case, before, after, mask):
    """Everything outside the view is bit-unchanged."""
    a, c = before.view(torch.int32)[~mask], after.view(torch.int32)[~mask]
    bad = a != c
    if bool(bad.any()):
        first = int(torch.nonzero(~mask).reshape(-1)[int(torch.nonzero(bad).reshape(-1)[0])])
        raise AssertionError(f"{case.id}: {int(bad.sum())} elements outside the C view changed, first at buffer "
                             f"offset {first}")


# ------------------------------------------------------------------------------------------ the table
def nt_name(bm, bn, a, bmode, pro, sk, bf=False):
    return f"gemm_nt_kernel<{bm}, {bn}, {a}, {bmode}, {b(pro)}, {b(sk)}, {b(bf)}>"


def nts_name(bm, bn, a, bmode, sk, terms, pro=False):
    return f"gemm_nts_kernel<{bm}, {bn}, {a}, {bmode}, {b(sk)}, {terms}, {b(pro)}>"


def nt8_name(a, pro, sk):
    return f"gemm_nt8_kernel<{a}, {b(pro)}, {b(sk)}>"


def _dense_geom(tile, a, bmode, m=None):
    """The issue's starting shapes: an interior tile, a ragged last tile in M and in N, several k-tiles and a
    k tail; M % 4 == 0 for A stored as k rows."""
    bm, bn = TILE_DIMS[tile]
    M = {64: 70, 128: 131}[bm] if a == 0 else {64: 72, 128: 132}[bm]
    return ("dense", m or M, {64: 68, 128: 132}[bn], 100)


def _conv_geom(tile, cfg, variant=None):
    """12 x 12 output pixels (144 rows): 3x3 / Cin 32 at stride 1 (plain) and stride 2 (full); 1x1 / Cin 64."""
    cout = {64: 68, 128: 132}[TILE_DIMS[tile][1]]
    if variant == "1x1":
        return ("conv", 1, 12, 12, 64, 1, 1, 0, cout)
    return ("conv", 1, 12, 12, 32, 3, 1, 1, cout) if cfg == "plain" else ("conv", 1, 24, 24, 32, 3, 2, 1, cout)


def _arm_geom(tile, a, bmode, cfg):
    if bmode == 2:
        return ("wgrad", 1, 12, 12, 16, 3, 1, 1, 132)
    if a == 4:
        return ("conv1", 1, 24, 24, {64: 68, 128: 132}[TILE_DIMS[tile][1]])
    if a == 2:
        return _conv_geom(tile, cfg)
    return _dense_geom(tile, a, bmode)


def _nt_family(cases, family, flags, arms, namer, tiles=(TILE_64, TILE_128x64, TILE_128)):
    """Every arm x tile x (stream-K, data-parallel) x (plain, full) of one launch helper of gemm_nt.hip."""
    for tile in tiles:
        bm, bn = (128, 128) if tile == TILE_W8 else TILE_DIMS[tile]
        gt = TILE_128 if tile == TILE_W8 else tile
        for (a, bmode, pro) in arms:
            for sk in (True, False):
                for cfg in ("plain", "full"):
                    geom = _arm_geom(gt, a, bmode, cfg)
                    dense = a in (0, 1) and bmode in (0, 1)
                    kw = dict(family=family, amode=a, bmode=bmode, tile=tile, flags=flags, cfg=cfg, pro=pro, sk=sk,
                              geoms=(geom,), expect=namer(bm, bn, a, bmode, pro, sk), stats=True,
                              a_remap=cfg == "full" and dense, c_remap=cfg == "full")
                    api = "sk" if sk else "gemm"
                    if not sk and pro and flags:
                        # capmi_gemm_ex sends prologue problems to the fp32 kernel: the data-parallel form of
                        # this arm is reached through a k-split (module docstring), plain configuration only
                        if cfg == "full":
                            continue
                        kw.update(ksplits=(2,), stats=False)
                        api = "sk"
                    cid = f"{family}-{bm}x{bn}{'w8' if tile == TILE_W8 else ''}-a{a}b{bmode}{'p' if pro else ''}-" \
                          f"{'sk' if sk else 'dp'}-{cfg}"
                    cases.append(Case(id=cid, api=api, **kw))


def _extra_dense(cases, family, flags, namer, a=0, bmode=0):
    """Per family: M = 1, and M in (64, 128) on a 128-row tile (the second 64-row statistics slice partial)."""
    for m, tile, sk in ((1, TILE_64, True), (1, TILE_128, False), (100, TILE_128, True), (100, TILE_128, False)):
        bm, bn = TILE_DIMS[tile]
        mm = m if a == 0 else 4 * ((m + 3) // 4)
        geom = ("dense", mm, {64: 68, 128: 132}[bn], 100)
        cases.append(Case(id=f"{family}-{bm}x{bn}-a{a}b{bmode}-M{mm}-{'sk' if sk else 'dp'}-full", family=family,
                          api="sk" if sk else "gemm", amode=a, bmode=bmode, tile=tile, flags=flags, cfg="full",
                          geoms=(geom,), expect=namer(bm, bn, a, bmode, False, sk), sk=sk, stats=True,
                          c_remap=m > 1))


def _x3_cases(cases):
    """gemm_x3 / x3p / x3d (dense and conv): the store-only epilogue (plain, plain + beta 1: whole column tiles,
    N = 128 or 64) and the general one (full: N ragged). Stream-K needs >= 8 k-tiles (K >= 256); the
    data-parallel form of the same problem is the launch without a workspace."""
    def add(fam, flags, a, pro, bn, sk, cfg, expect, geom, tile=TILE_AUTO):
        remap = cfg == "full" and geom[0] == "dense"      # statistics and the C remap exclude each other here
        cases.append(Case(id=f"{fam}-bn{bn}-a{a}{'p' if pro else ''}-{'sk' if sk else 'dp'}-{cfg}", family=fam,
                          api="sk", amode=a, bmode=0, tile=tile, flags=flags, cfg=cfg, geoms=(geom,), expect=expect,
                          sk=sk, pro=pro, stats=not remap, c_remap=remap, ws=sk))
    for bn in (128, 64):
        tile = TILE_AUTO if bn == 128 else TILE_128x64
        for cfg in ("plain", "plain_beta1", "full"):
            n = bn if cfg != "full" else bn + 4
            conv = ("conv", 1, 12, 12, 32, 3, 1, 1, n) if cfg != "full" else ("conv", 1, 24, 24, 32, 3, 2, 1, n)
            for sk in (True, False):
                add("x3", X3, 0, False, bn, sk, cfg, f"gemm_x3_kernel<{bn}, 0, false, {b(sk)}>",
                    ("dense", 131, n, 256), tile)
                for pro in (False, True):
                    add("x3", X3, 2, pro, bn, sk, cfg, f"gemm_x3_kernel<{bn}, 2, {b(pro)}, {b(sk)}>", conv, tile)
    for cfg in ("plain", "plain_beta1", "full"):
        n = 128 if cfg != "full" else 132
        conv = ("conv", 2, 12, 12, 32, 3, 1, 1, n) if cfg != "full" else ("conv", 2, 24, 24, 32, 3, 2, 1, n)
        for sk in (True, False):
            for a, geom in ((0, ("dense", 300, n, 256)), (2, conv)):
                add("x3p", X3P, a, False, 128, sk, cfg, f"gemm_x3p_kernel<{a}, {b(sk)}, 32, false, false>", geom)
                for pro in (False, True):
                    if cfg == "plain_beta1" and sk:
                        continue  # x3d runs C = A.B + beta C data-parallel whatever the grid (plan_x3d)
                    add("x3d", X3D, a, pro, 128, sk, cfg, f"gemm_x3p_kernel<{a}, {b(sk)}, 32, true, {b(pro)}>", geom)


def _x3w_cases(cases):
    """gemm_x3w / gemm_w16: alpha / beta only. The k-split form (SK = true) needs alpha 1, beta 0 and >= 8
    k-tiles of 32 pixels; N = 128 takes the store-only epilogue. M % 4 == 0 is the family's own rule, so it has no
    M = 1 case; M = 100 (inside its single 256-row tile; the family writes no statistics) is added in _build."""
    for bf16 in (False, True):
        fam, kern = ("w16", "gemm_w16_kernel") if bf16 else ("x3w", "gemm_x3w_kernel")
        flags = X3W | (BF16 if bf16 else 0)
        for bmode in (1, 2):
            for cfg, split, pro in (("plain", True, False), ("plain", False, False), ("full", False, bmode == 2),
                                    ("plain_beta1", False, False)):
                if bmode == 2:
                    cin = 16 if cfg != "plain_beta1" else 128
                    k = 3 if cfg != "plain_beta1" else 1
                    geom = ("wgrad", 2 if split else 1, 12, 12, cin, k, 1, k // 2, 132)
                else:
                    geom = ("dense", 132, 128 if cfg == "plain_beta1" else 68, 292 if split else 100)
                cases.append(Case(id=f"{fam}-b{bmode}{'p' if pro else ''}-{'split' if split else 'one'}-{cfg}",
                                  family=fam, api="sk", amode=1, bmode=bmode, tile=TILE_AUTO, flags=flags, cfg=cfg,
                                  geoms=(geom,), expect=f"{kern}<{bmode}, {b(split)}>", sk=split, pro=pro,
                                  fields="alpha_beta"))


def _generic_cases(cases):
    """gemm.hip's generic kernel: the scalar-load arm (K % 4 != 0 and odd leading dimensions), and the modes
    the v2 kernel does not take (A stored as k rows x W[N][K]; the NCHW gather of conv1), both tile sizes."""
    for tile, (bm, wm) in ((TILE_64, (64, 32)), (TILE_128, (128, 64))):
        n = {64: 68, 128: 132}[bm]
        for cfg in ("plain", "full"):
            for name, a, geom, vec, unal in (
                    ("scalar", 0, ("dense", {64: 70, 128: 131}[bm], n, 102), False, True),
                    ("a1b0", 1, ("dense", {64: 72, 128: 132}[bm], n, 100), True, False),
                    ("nchw", 3, ("conv", 1, 24, 24, 3, 7, 2, 3, n), False, True)):
                cases.append(Case(id=f"generic-{bm}-{name}-{cfg}", family="generic", api="gemm", amode=a, bmode=0,
                                  tile=tile, flags=0, cfg=cfg, geoms=(geom,), stats=True, unaligned=unal,
                                  a_remap=cfg == "full" and a == 1, c_remap=cfg == "full",
                                  expect=f"gemm_kernel<{bm}, {bm}, {wm}, {wm}, {a}, 0, {b(vec)}>"))


def _build():
    cases = []
    _generic_cases(cases)
    nt_arms = [(0, 0, False), (0, 1, False), (1, 1, False), (2, 0, False), (2, 0, True), (4, 0, False),
               (1, 2, False), (1, 2, True)]
    _nt_family(cases, "nt", 0, nt_arms, nt_name)
    _nt_family(cases, "nt8", 0, [(4, 0, False), (0, 0, False), (2, 0, True), (2, 0, False)],
               lambda bm, bn, a, bmode, pro, sk: nt8_name(a, pro, sk), tiles=(TILE_W8,))
    _nt_family(cases, "nts3", SPLIT3, nt_arms,
               lambda bm, bn, a, bmode, pro, sk: nts_name(bm, bn, a, bmode, sk, 3, pro))
    _nt_family(cases, "nts1", BF16, [(0, 1, False), (1, 1, False)],
               lambda bm, bn, a, bmode, pro, sk: nts_name(bm, bn, a, bmode, sk, 1, pro))
    _nt_family(cases, "bf16", BF16, [(4, 0, False), (0, 0, False), (2, 0, True), (2, 0, False)],
               lambda bm, bn, a, bmode, pro, sk: nt_name(bm, bn, a, bmode, pro, sk, True))
    # the 1x1 conv (two k-tiles, stride 1, no padding) on every tile of the fp32 and three-term conv arms
    for fam, flags, namer in (("nt", 0, nt_name),
                              ("nts3", SPLIT3, lambda bm, bn, a, bmode, pro, sk: nts_name(bm, bn, a, bmode, sk, 3, pro))):
        for tile in (TILE_64, TILE_128x64, TILE_128):
            bm, bn = TILE_DIMS[tile]
            cases.append(Case(id=f"{fam}-{bm}x{bn}-a2b0-1x1-sk-full", family=fam, api="sk", amode=2, bmode=0,
                              tile=tile, flags=flags, cfg="full", geoms=(_conv_geom(tile, "full", "1x1"),),
                              expect=namer(bm, bn, 2, 0, False, True), sk=True, stats=True, c_remap=True))
    _extra_dense(cases, "nt", 0, nt_name)
    _extra_dense(cases, "nts3", SPLIT3, lambda bm, bn, a, bmode, pro, sk: nts_name(bm, bn, a, bmode, sk, 3, pro))
    _extra_dense(cases, "nts1", BF16, lambda bm, bn, a, bmode, pro, sk: nts_name(bm, bn, a, bmode, sk, 1, pro),
                 bmode=1)
    _extra_dense(cases, "bf16", BF16, lambda bm, bn, a, bmode, pro, sk: nt_name(bm, bn, a, bmode, pro, sk, True))
    for m, sk in ((1, False), (100, True)):
        cases.append(Case(id=f"nt8-a0b0-M{m}-{'sk' if sk else 'dp'}-full", family="nt8", api="sk" if sk else "gemm",
                          amode=0, bmode=0, tile=TILE_W8, flags=0, cfg="full", geoms=(("dense", m, 132, 100),),
                          expect=nt8_name(0, False, sk), sk=sk, stats=True, c_remap=m > 1))
    for m in (1, 100):
        cases.append(Case(id=f"generic-64-scalar-M{m}-full", family="generic", api="gemm", amode=0, bmode=0,
                          tile=TILE_64, flags=0, cfg="full", geoms=(("dense", m, 68, 102),), stats=True,
                          unaligned=True, expect="gemm_kernel<64, 64, 32, 32, 0, 0, false>"))
    _x3_cases(cases)
    for fam, flags, geom, kern in (("x3", X3, ("dense", 1, 132, 256), "gemm_x3_kernel<128, 0, false, true>"),
                                   ("x3", X3, ("dense", 100, 132, 256), "gemm_x3_kernel<128, 0, false, true>"),
                                   ("x3p", X3P, ("dense", 1, 132, 256), "gemm_x3p_kernel<0, true, 32, false, false>"),
                                   ("x3d", X3D, ("dense", 1, 132, 256), "gemm_x3p_kernel<0, true, 32, true, false>"),
                                   ("x3d", X3D, ("dense", 100, 132, 256), "gemm_x3p_kernel<0, true, 32, true, false>")):
        cases.append(Case(id=f"{fam}-a0-M{geom[1]}-sk-full", family=fam, api="sk", amode=0, bmode=0, tile=TILE_AUTO,
                          flags=flags, cfg="full", geoms=(geom,), expect=kern, sk=True, stats=True))
    cases.append(Case(id="x3p-a0-M100-sk-full", family="x3p", api="sk", amode=0, bmode=0, tile=TILE_AUTO, flags=X3P,
                      cfg="full", geoms=(("dense", 100, 132, 256),),
                      expect="gemm_x3p_kernel<0, true, 32, false, false>", sk=True, stats=True))
    _x3w_cases(cases)
    for fam, flags, kern in (("x3w", X3W, "gemm_x3w_kernel"), ("w16", X3W | BF16, "gemm_w16_kernel")):
        cases.append(Case(id=f"{fam}-b1-M100-full", family=fam, api="sk", amode=1, bmode=1, tile=TILE_AUTO,
                          flags=flags, cfg="full", geoms=(("dense", 100, 68, 100),), expect=f"{kern}<1, false>",
                          fields="alpha_beta"))
    # the families whose contract is the product alone (statistics optional)
    cases.append(Case(id="x3s-dense-plain", family="x3s", api="sk", amode=0, bmode=0, tile=TILE_AUTO, flags=X3S,
                      cfg="plain", geoms=(("dense", 70, 64, 64),), expect="gemm_x3s_kernel<1, false>", stats=True,
                      ws=False))
    cases.append(Case(id="x3c-conv-plain", family="x3c", api="sk", amode=2, bmode=0, tile=TILE_AUTO, flags=X3C,
                      cfg="plain", geoms=(("conv", 2, 12, 12, 32, 3, 1, 1, 64),), expect="gemm_x3c_kernel<true>",
                      pro=True, stats=True, ws=False))
    # grouped launches: two problems sharing A with different k-splits, the bias in slab 0 only
    for fam, flags, kern in (("nt", 0, nt_name(64, 64, 0, 0, False, False)),
                             ("nts3", SPLIT3, nts_name(64, 64, 0, 0, False, 3))):
        cases.append(Case(id=f"{fam}-grouped-ksplit", family=fam, api="gemm", amode=0, bmode=0, tile=TILE_64,
                          flags=flags, cfg="plain", geoms=(("dense", 70, 68, 200), ("dense", 70, 132, 200)),
                          ksplits=(2, 3), expect=kern, fields="bias"))
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"

# every field a family's documented contract omits (include/capmi.h): refused with CAPMI_EINVAL, nothing launched.
# refuse = alpha / beta / bias / relu set that epilogue field; stats / ksplit / a_remap / c_remap set the Case's own.
def _refusals():
    out = []
    x3w = dict(family="x3w", api="sk", amode=1, bmode=1, tile=TILE_AUTO, flags=X3W, cfg="plain",
               geoms=(("dense", 132, 68, 100),), expect="")
    x3s = dict(family="x3s", api="sk", amode=0, bmode=0, tile=TILE_AUTO, flags=X3S, cfg="plain",
               geoms=(("dense", 70, 64, 64),), expect="", ws=False)
    x3c = dict(family="x3c", api="sk", amode=2, bmode=0, tile=TILE_AUTO, flags=X3C, cfg="plain",
               geoms=(("conv", 2, 12, 12, 32, 3, 1, 1, 64),), expect="", ws=False)
    for base, fields in ((x3w, ("bias", "relu", "stats", "ksplit", "a_remap", "c_remap")),
                         (x3s, ("alpha", "beta", "bias", "relu", "ksplit", "a_remap", "c_remap")),
                         (x3c, ("alpha", "beta", "bias", "relu", "ksplit", "c_remap"))):
        for f in fields:
            kw = dict(base, refuse=f)
            if f == "stats":
                kw["stats"] = True
            elif f == "ksplit":
                kw["ksplits"] = (2,)
            elif f in ("a_remap", "c_remap"):
                kw[f] = True
            out.append(Case(id=f"{base['family']}-refuses-{f}", **kw))
    return out


REFUSALS = _refusals()

# launch sites of csrc/gemm_nt.hip that no host path reaches (kernel, AMODE, BMODE, PRO, TERMS) -> why
UNREACHABLE = {
    ("gemm_nt_kernel", 1, 0, False, 0): "plan_nt_group (gemm_plan.hip) keeps A-as-k-rows x W[N][K] off the v2 "
                                        "kernel (nt_ok): it runs the generic kernel, which the generic-*-a1b0 "
                                        "cases pin",
    ("gemm_nts_kernel", 0, 0, False, 1): "launch_bmbn sends the bf16 forward modes (terms 1, B = W[N][K]) to "
                                         "launch_sk_bf16, which the bf16-* cases pin",
}


# ------------------------------------------------------------------------------------------ launch-site scan
def _eval_targ(text, env):
    """One template argument of a launch site: a literal, a helper template parameter, or `P == v ? x : y`."""
    text = text.strip()
    m = re.fullmatch(r"(\w+) == (\d+) \? (\w+) : (\w+)", text)
    if m:
        return _eval_targ(m.group(3) if env[m.group(1)] == int(m.group(2)) else m.group(4), env)
    m = re.fullmatch(r"(\w+) == (\d+)", text)
    if m:
        return env[m.group(1)] == int(m.group(2))
    if text in env:
        return env[text]
    if text in ("true", "false"):
        return text == "true"
    return int(text)


def launch_sites(source):
    """The CAPMI_KLAUNCH sites of the launch helpers of csrc/gemm_nt.hip, each expanded over the template
    contexts its helper is instantiated with: [(name as the runtime prints it, key, 'file line: text')].
    key = (kernel, AMODE, BMODE, PRO, TERMS). A site guarded by `TERMS == 3 &&` is dead in a TERMS = 1 helper."""
    lines = source.splitlines()
    tiles = sorted({(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"launch_bmbn<(\d+), (\d+)>\(", source)})
    assert tiles, "no launch_bmbn instantiation found"
    helper, out = None, []
    for no, line in enumerate(lines, 1):
        m = re.match(r"void (launch_\w+)\(", line)
        if m:
            helper = m.group(1)
        if line.startswith("}"):
            helper = None
        m = re.search(r"CAPMI_KLAUNCH\(\((\w+)<(.*)>\), g, b, 0, s, a\);", line)
        if not m:
            assert "CAPMI_KLAUNCH" not in line, f"gemm_nt.hip:{no}: a launch site this scan cannot read: {line.strip()}"
            continue
        where = f"gemm_nt.hip:{no}: {line.strip()}"
        assert helper in ("launch_sk", "launch_nts", "launch_nt8", "launch_sk_bf16"), f"{where}: unknown helper {helper}"
        cond = lines[no - 2]
        kernel, targs = m.group(1), [t for t in m.group(2).split(", ")]
        for bm, bn in ([(128, 128)] if helper == "launch_nt8" else tiles):
            for terms in ((1, 3) if helper == "launch_nts" else (0,)):
                if terms == 1 and "TERMS == 3 &&" in cond:
                    continue
                for sk in (True, False):
                    env = dict(BM=bm, BN=bn, SK=sk, TERMS=terms)
                    v = [_eval_targ(t, env) for t in targs]
                    if kernel == "gemm_nt_kernel":
                        v = v + [False] * (7 - len(v))
                        name, key = nt_name(*v), (kernel, v[2], v[3], v[4], 0)
                    elif kernel == "gemm_nts_kernel":
                        v = v + [False] * (7 - len(v))
                        name, key = nts_name(v[0], v[1], v[2], v[3], v[4], v[5], v[6]), (kernel, v[2], v[3], v[6], v[5])
                    else:
                        assert kernel == "gemm_nt8_kernel", where
                        name, key = nt8_name(*v), (kernel, v[0], 0, v[1], 0)
                    out.append((name, key, where))
    return out
