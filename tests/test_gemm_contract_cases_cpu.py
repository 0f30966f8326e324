"""CPU: the case table, the fp64 restatement and the comparison rules of the GEMM contract tests
(tests/gemm_contract_cases.py, which tests/test_gpu_gemm_contract.py runs every GEMM kernel form against).

  * the restatement (index arithmetic: the row remaps, the implicit im2col, the k ranges of k-split slabs)
    agrees with torch fp64 built independently: F.conv2d for the conv modes, autograd for the weight gradient,
    matmul on reshaped views for the dense modes, elementwise ops for the epilogue;
  * every case's inputs satisfy its own preconditions (alignment rules of its mode; a full case's relu clips
    between a quarter and three quarters of C, beta*C0 is of the product's size; the nt tiles have an interior
    tile, ragged last tiles and a k tail);
  * the rules have teeth: statistics one slot off, a beta == 0 path that reads C, a touched canary each fail
    the comparison the GPU test makes;
  * completeness: every CAPMI_KLAUNCH site of the launch helpers of csrc/gemm_nt.hip is named by a case, for
    every tile and in both the stream-K and the data-parallel form, or is listed as unreachable with the reason;
  * the planner (capmi_gemm_sk_plan, no GPU work) agrees with the instantiation each stream-K-API case names, and
    refuses every refusal case. This last test needs the built libcapmi.so (as tests/test_lib_cpu.py does); the
    others need torch alone."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import gemm_contract_cases as GC

F64 = torch.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = GC.CASES + GC.REFUSALS


@functools.lru_cache(maxsize=None)
def _data(cid):
    case = GC.BY_ID.get(cid) or next(c for c in GC.REFUSALS if c.id == cid)
    inp = GC.make_inputs(case)
    return case, inp, GC.gemm_contract_ref(case, inp)


# ------------------------------------------------------------------------------------------ independent torch
def _rows(buf, rows, width, r1, n):
    """The first n logical rows of a [rows x width] buffer, through torch views instead of offsets."""
    m = buf.reshape(rows, width)
    if r1 > 0:
        m = m.view(r1, rows // r1, width).permute(1, 0, 2).reshape(rows, width)
    return m[:n]


def _c_logical(L, buf, z):
    start = L.c_off - 4 + z * L.c_split_stride
    phys = buf[start: start + L.c_rows * L.c_width].reshape(L.c_rows, L.c_width)[:, 4: 4 + L.N]
    if L.c_r1 > 0:
        phys = phys.reshape(L.c_r1, L.c_rows // L.c_r1, L.N).permute(1, 0, 2).reshape(L.c_rows, L.N)
    return phys[:L.M]


def _independent(case, L, p, k0, k1):
    """(product, magnitude product) over k in [k0, k1), fp64, from torch's own ops."""
    bf16 = case.family in GC.BF16_FAMILIES
    rnd = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t.double())

    def pro(x):  # channels last
        if not case.pro:
            return x.double()
        if bf16:
            return torch.relu(torch.addcmul(p["in_shift"], x, p["in_scale"])).double()
        return torch.relu(torch.addcmul(p["in_shift"].double(), x.double(), p["in_scale"].double()))
    g = L.geo
    if case.bmode == 2:  # dW = autograd's weight gradient of conv2d(x) under the output gradient dY
        x = rnd(pro(p["B"])).permute(0, 3, 1, 2)
        dY = rnd(_rows(p["A"], L.a_rows, L.a_width, L.a_r1, L.K)[:, :L.M]).clone()
        dY[:k0] = 0
        dY[k1:] = 0
        dY = dY.reshape(g["N"], g["Ho"], g["Wo"], L.M).permute(0, 3, 1, 2)
        outs = []
        for xx, dd in ((x, dY), (x.abs(), dY.abs())):
            w = torch.zeros(L.M, g["Cin"], g["KH"], g["KW"], dtype=F64, requires_grad=True)
            F.conv2d(xx, w, stride=g["stride"], padding=g["pad"]).backward(dd)
            outs.append(w.grad.permute(0, 2, 3, 1).reshape(L.M, L.N))
        return outs
    if case.amode >= 2:
        wflat = rnd(p["B"][:, :L.K]).clone()
        wflat[:, :k0] = 0
        wflat[:, k1:] = 0
        if case.amode == 3:
            x, w = rnd(p["A"]), wflat.reshape(L.N, g["Cin"], g["KH"], g["KW"])
        else:
            x = rnd(pro(p["A"])).permute(0, 3, 1, 2)
            w = wflat.reshape(L.N, g["KH"], g["KW"], g["Cin"]).permute(0, 3, 1, 2)
        return [F.conv2d(xx, ww, stride=g["stride"], padding=g["pad"]).permute(0, 2, 3, 1).reshape(L.M, L.N)
                for xx, ww in ((x, w), (x.abs(), w.abs()))]
    if case.amode == 0:
        A = _rows(p["A"], L.a_rows, L.a_width, L.a_r1, L.M)[:, :L.K]
        A = rnd(pro(A))
    else:
        A = rnd(_rows(p["A"], L.a_rows, L.a_width, L.a_r1, L.K)[:, :L.M]).T
    B = rnd(p["B"][:, :L.K]).T if case.bmode == 0 else rnd(p["B"][:, :L.N])
    return [A[:, k0:k1] @ B[k0:k1], A[:, k0:k1].abs() @ B[k0:k1].abs()]


@pytest.mark.parametrize("cid", [c.id for c in ALL])
def test_restatement_is_torch(cid):
    case, inp, ref = _data(cid)
    alpha, aptr, beta, relu, _, _ = GC.epilogue(case)
    eff = alpha * (aptr if aptr is not None else 1.0)
    for i, p in enumerate(inp):
        L = GC.layout(case, i)
        assert len(L.k_ranges) == L.ksplit and L.k_ranges[0][0] == 0 and L.k_ranges[-1][1] == L.K
        for z, (k0, k1) in enumerate(L.k_ranges):
            prod, mag = _independent(case, L, p, k0, k1)
            v, m = eff * prod, abs(eff) * mag
            if z == 0:
                for name in ("bias", "bias2"):
                    if p[name] is not None:
                        v, m = v + p[name].double(), m + p[name].double().abs()
            if beta != 0.0:
                c0 = _c_logical(L, p["C"], z).double()
                v, m = v + beta * c0, m + abs(beta) * c0.abs()
            if relu:
                v = v.clamp_min(0)
            torch.testing.assert_close(ref[i][0][z], v, rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(ref[i][1][z], m, rtol=1e-12, atol=1e-12)
            # the view the offsets address is the view torch's reshapes address
            buf = torch.arange(L.c_numel, dtype=F64)
            assert torch.equal(buf[GC.c_offsets(L)[z]], _c_logical(L, buf, z))


# ------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("cid", [c.id for c in ALL])
def test_case_preconditions(cid):
    case, inp, ref = _data(cid)
    alpha, aptr, beta, relu, _, _ = GC.epilogue(case)
    for i, p in enumerate(inp):
        L = GC.layout(case, i)
        view = GC.c_view_mask(case, i)
        assert int(view.sum()) == L.ksplit * L.M * L.N, "the remap addresses an element twice"
        inside, outside = p["C"][view], p["C"][~view]
        assert bool((outside == GC.CANARY).all()) and outside.numel() >= (GC.GUARD_ROWS + 1) * L.c_width
        assert bool(torch.isnan(inside).all()) if beta == 0.0 else bool(torch.isfinite(inside).all())
        assert L.ldc > L.N and L.c_off % 4 == 0
        if case.c_remap and L.M > 1:
            assert L.c_rows >= L.M and L.c_r1 == GC.R1
        # alignment rules of the mode (include/capmi.h)
        if not case.unaligned:
            if case.amode in (0, 1):
                assert L.lda % 4 == 0 and L.a_s2 % 4 == 0
            if case.amode == 0:
                assert L.K % 4 == 0
            if case.amode == 1:
                assert L.M % 4 == 0
            if case.bmode == 0:
                assert L.ldb % 4 == 0 and L.ldb >= L.K
            if case.bmode == 1:
                assert L.N % 4 == 0 and L.ldb % 4 == 0
        if case.amode == 2 and case.family != "generic":
            assert L.geo["Cin"] % 32 == 0
        if case.bmode == 2:
            assert L.geo["Cin"] % 4 == 0 and case.amode == 1
        if case.family in ("x3", "x3p", "x3d", "x3s", "x3c"):
            assert L.K % 32 == 0 and L.ldb % 8 == 0
        if case.family == "x3p" and case.amode == 0:
            assert L.lda % 8 == 0
        if case.stats:
            assert L.ksplit == 1 and p["stats"].shape[0] == L.stat_slices + 2
        if case.cfg == "full" and case.fields == "all" and not case.refuse:
            exp = ref[i][0]
            clipped = float((exp == 0).double().mean())
            assert 0.25 <= clipped <= 0.75, f"relu clips {clipped:.2f} of C"
        if beta != 0.0 and not case.refuse:
            Al, Bl = GC.operands(case, L, p)
            eff = abs(alpha * (aptr if aptr is not None else 1.0))
            r = float((beta * inside.double()).pow(2).mean().sqrt() / (eff * (Al @ Bl)).pow(2).mean().sqrt())
            assert 0.5 <= r <= 2.0, f"rms(beta*C0) / rms(alpha*A.B) = {r:.3g}"


def test_table_covers_the_tile_edges():
    """The main cases of the v2 kernel's families: at least one interior tile, a ragged last tile in M and in
    N, several k-tiles and (dense and conv1 modes) a k tail, in one launch; the extra cases M = 1 and a partial
    second statistics slice of a 128-row tile; nothing larger than a few hundred rows."""
    for c in GC.CASES:
        for i in range(len(c.geoms)):
            L = GC.layout(c, i)
            assert max(L.M, L.N) <= 320 and L.K <= 320, c.id
        if c.family in ("nt", "nt8", "nts3", "nts1", "bf16") and "-M" not in c.id and "grouped" not in c.id:
            L = GC.layout(c)
            bm, bn = (128, 128) if c.tile == GC.TILE_W8 else GC.TILE_DIMS[c.tile]
            assert L.M > bm and L.M % bm and L.N > bn and L.N % bn, c.id
            assert L.K > 32, c.id
            if c.amode in (0, 1, 4) or c.bmode == 2:
                assert L.K % 32, c.id
    for fam in ("generic", "nt", "nt8", "nts3", "nts1", "bf16", "x3", "x3p", "x3d", "x3w", "w16"):
        ms = {GC.layout(c).M for c in GC.CASES if c.family == fam}
        if fam not in ("x3w", "w16"):  # M % 4 == 0 is that family's own rule
            assert 1 in ms, fam
        assert any(64 < m < 128 for m in ms), fam


# ------------------------------------------------------------------------------------------ teeth
def test_rules_have_teeth():
    case, inp, ref = _data("nt-128x128-a0b0-sk-full")
    L = GC.layout(case)
    exp, bound = ref[0]
    stored = exp[0].float()
    GC.check_result(case, stored, exp[0], bound[0])
    # statistics: right, then every slice written one slot further on
    v = stored.double()
    st = torch.full((L.stat_slices + 2, L.N, 2), GC.CANARY)
    for s in range(L.stat_slices):
        rows = v[64 * s: 64 * (s + 1)]
        st[s, :, 0], st[s, :, 1] = rows.sum(0).float(), (rows * rows).sum(0).float()
    GC.check_stats(case, L, stored, st)
    with pytest.raises(AssertionError, match="stats slice 0"):
        GC.check_stats(case, L, stored, torch.roll(st, 1, 0))
    swapped = st.clone()
    swapped[[0, 1]] = st[[1, 0]]
    with pytest.raises(AssertionError, match="stats slice"):
        GC.check_stats(case, L, stored, swapped)  # the sum over slices would still agree
    with pytest.raises(AssertionError, match="past slice"):
        late = st.clone()
        late[L.stat_slices] = 0.0
        GC.check_stats(case, L, stored, late)
    # a beta == 0 path that reads C: the NaN prefill reaches the result
    pcase, pinp, pref = _data("nt-128x128-a0b0-sk-plain")
    pexp, pbound = pref[0]
    PL = GC.layout(pcase)
    c0 = pinp[0]["C"][GC.c_offsets(PL)[0]]
    with pytest.raises(AssertionError, match="outside"):
        GC.check_result(pcase, pexp[0].float() + 0.0 * c0, pexp[0], pbound[0])
    # one wrong column inside the view, one touched canary outside it
    bad = stored.clone()
    bad[-1, -1] += 1e-3 * float(bound[0][-1, -1]) + 1e-3
    with pytest.raises(AssertionError, match="outside"):
        GC.check_result(case, bad, exp[0], bound[0])
    mask = GC.c_view_mask(case)
    after = inp[0]["C"].clone()
    after[mask] = 0.0
    GC.check_canaries(case, inp[0]["C"], after, mask)
    after[int(torch.nonzero(~mask)[7])] = 0.0
    with pytest.raises(AssertionError, match="outside the C view"):
        GC.check_canaries(case, inp[0]["C"], after, mask)


# ------------------------------------------------------------------------------------------ completeness
def _sites():
    with open(os.path.join(REPO, "image-captioning-with-different-decoders_amd", "csrc", "gemm_nt.hip")) as f:
        return GC.launch_sites(f.read())


def test_every_launch_site_has_a_case():
    sites = _sites()
    assert len({w for _, _, w in sites}) >= 25, "the scan lost launch sites"
    covered = {c.expect for c in GC.CASES}
    missing, stale = [], set(GC.UNREACHABLE)
    for name, key, where in sites:
        if key in GC.UNREACHABLE:
            stale.discard(key)
            assert name not in covered, f"{name} is listed unreachable but a case expects it"
            continue
        if name not in covered:
            missing.append(f"{where}  ->  {name}")
    assert not missing, "launch sites of gemm_nt.hip without a case:\n" + "\n".join(missing)
    assert not stale, f"UNREACHABLE lists sites gemm_nt.hip no longer has: {stale}"
    # and the other way round: every v2-kernel name a case expects is a site of the file
    names = {n for n, _, _ in sites}
    for c in GC.CASES:
        if c.expect.startswith(("gemm_nt_kernel", "gemm_nts_kernel", "gemm_nt8_kernel")):
            assert c.expect in names, f"{c.id} expects {c.expect}, which gemm_nt.hip does not launch"


def test_a_new_launch_site_fails_the_scan():
    with open(os.path.join(REPO, "image-captioning-with-different-decoders_amd", "csrc", "gemm_nt.hip")) as f:
        src = f.read()
    old = "    CAPMI_KLAUNCH((gemm_nt8_kernel<0, false, SK>), g, b, 0, s, a);"
    assert old in src
    sites = GC.launch_sites(src.replace(old, old + "\n  else if (amode == 1)\n"
                                        "    CAPMI_KLAUNCH((gemm_nt8_kernel<1, false, SK>), g, b, 0, s, a);"))
    covered = {c.expect for c in GC.CASES}
    new = [w for n, k, w in sites if n not in covered and k not in GC.UNREACHABLE]
    assert new and all("gemm_nt8_kernel<1, false, SK>" in w for w in new)


def test_both_forms_of_every_instantiation():
    """Stream-K and data-parallel, plain and full, per (family, kernel arm, tile) of the v2 kernel."""
    seen = {}
    for c in GC.CASES:
        if c.family in ("nt", "nt8", "nts3", "nts1", "bf16") and "grouped" not in c.id:
            seen.setdefault((c.family, c.amode, c.bmode, c.pro, c.tile), set()).add((c.sk, c.cfg))
    for key, forms in seen.items():
        assert {(True, "plain"), (True, "full"), (False, "plain")} <= forms, (key, forms)
        if not (key[3] and key[0] in ("nts3", "bf16")):  # (module docstring: the k-split route is plain only)
            assert (False, "full") in forms, (key, forms)


# ------------------------------------------------------------------------------------------ the planner
def _plan_problem(case):
    from capmi._lib import GemmProblem
    L = GC.layout(case)
    alpha, aptr, beta, relu, b1, b2 = GC.epilogue(case)
    fake = 0x10000  # never dereferenced by a plan query
    p = GemmProblem()
    p.M, p.N, p.K, p.ksplit = L.M, L.N, L.K, L.ksplit
    p.A, p.lda, p.a_r1, p.a_s2 = fake + (4 if case.unaligned else 0), L.lda, L.a_r1, L.a_s2
    p.B, p.ldb = fake, L.ldb
    p.C, p.ldc, p.c_r1, p.c_s2, p.c_split_stride = fake, L.ldc, L.c_r1, L.c_s2, L.c_split_stride
    p.bias, p.bias2 = (fake if b1 else None), (fake if b2 else None)
    p.alpha_ptr = fake if aptr is not None else None
    p.alpha, p.beta, p.relu = alpha, beta, int(relu)
    p.stats = fake if case.stats else None
    if L.geo:
        g = L.geo
        p.cN, p.cH, p.cW, p.cCin, p.cKH, p.cKW = g["N"], g["H"], g["W"], g["Cin"], g["KH"], g["KW"]
        p.cStride, p.cPad, p.cHo, p.cWo = g["stride"], g["pad"], g["Ho"], g["Wo"]
    if case.pro:
        p.in_scale = p.in_shift = fake
    return p


@pytest.mark.parametrize("cid", [c.id for c in ALL if c.api == "sk"])
def test_planner_names_the_expected_instantiation(cid):
    """capmi_gemm_sk_plan (host arithmetic only, 256 CUs assumed where no device answers) on the case's problem:
    the tile, stream-K or not, the generic fall-back and the workgroup size are the ones the case's expected
    kernel name states; a refusal case is refused by the planner with CAPMI_EINVAL."""
    from capmi._lib import lib
    case = GC.BY_ID.get(cid) or next(c for c in GC.REFUSALS if c.id == cid)
    p = _plan_problem(case)
    v = [ctypes.c_int(-1) for _ in range(5)]
    rc = lib.capmi_gemm_sk_plan(ctypes.byref(p), case.amode, case.bmode, case.tile, case.flags,
                                *[ctypes.byref(x) for x in v])
    if case.refuse:
        assert rc == GC.EINVAL
        return
    assert rc == 0, rc
    bm, bn, sk, generic, threads = (x.value for x in v)
    # (the plan of the x3 kernels assumes a workspace: their data-parallel cases are the launch without one)
    want_sk = case.sk or (case.family in ("x3", "x3p", "x3d") and not case.ws)
    if case.family == "x3d" and case.cfg == "plain_beta1":
        want_sk = False  # C = A.B + beta C: data-parallel whatever the grid (x3d_plan)
    assert bool(sk) == want_sk, (sk, case.sk)
    if case.family in ("nt", "nts3", "nts1", "bf16"):
        assert (bm, bn) == GC.TILE_DIMS[case.tile] and generic == 0 and threads == 256
        assert case.expect.startswith(("gemm_nt_kernel<%d, %d," % (bm, bn), "gemm_nts_kernel<%d, %d," % (bm, bn)))
    elif case.family == "nt8":
        assert (bm, bn, threads, generic) == (128, 128, 512, 0)
    elif case.family == "x3":
        assert (bm, threads) == (128, 512) and case.expect.startswith(f"gemm_x3_kernel<{bn},")
    elif case.family in ("x3p", "x3d"):
        assert (bm, bn, threads, generic) == (256, 128, 512, 32)
    elif case.family in ("x3w", "w16"):
        assert (bm, bn, threads) == (256, 128, 512) and (generic > 1) == case.sk
