"""Helper of tests/test_gemm_plan_table_cpu.py (not a test): a deterministic list of capmi_gemm_sk_plan queries and
the generator of tests/golden/gemm_plan_table.npz, one int row [rc, bm, bn, stream_k, generic, threads] per query
(the five outputs stay -1 where the query is refused).

The table pins what the host planner (csrc/gemm_plan.hip) answers on a 256-CU device with no CAPMI_* planner
variable set. It was written by the library built from the commit before the planner moved out of csrc/gemm.hip:

    CAPMI_LIB=<that build's libcapmi.so> python tests/gemm_plan_queries.py --write

Regenerate it only together with a deliberate change of a planning rule. Without --write the script prints a digest
of the rows (the one-off A/B of the CAPMI_* knobs: run it under each setting against two builds and compare).

The list: every accepted flag value and two refused combinations x (tiles 0-4 on the plain problem, and at the
automatic tile every epilogue / addressing variant that steers a branch of the planner) x
  * ResNet-101's convs at batch 1, 5 and 64 as NHWC convs (amode 2; conv1 as NHWC4, amode 4) and as conv weight
    gradients (amode 1, bmode 2),
  * the decoder's GEMM shapes in the four dense operand modes,
  * the launches of tests/gemm_contract_cases.py (their own layouts, modes and tiles)."""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "gemm_plan_table.npz")
FLAGS = (0, 1, 16, 2, 4, 8, 32, 64, 128, 129, 256)
REFUSED_FLAGS = (1 | 2, 1 | 16)
TILES = (0, 1, 2, 3, 4)
TILE_AUTO = 3
EINVAL, EALIGN, ERANGE = 1001, 1002, 1003
CUS = 256  # the device the table answers for
# 16-byte aligned stand-ins: the plan never dereferences an operand
PTR = dict(A=0x10000, B=0x20000, C=0x30000, bias=0x40000, alpha_ptr=0x50000, stats=0x60000, in_scale=0x70000,
           in_shift=0x80000)


def workspace_bytes(cus):
    """capmi_gemm_workspace_bytes() of a device with `cus` CUs (include/capmi.h)."""
    return ((cus * 4 + 1) * 4 + 255) // 256 * 256 + cus * 128 * 1024


# ------------------------------------------------------------------------------------------ shapes
def resnet101_convs():
    """(name, H, Cin, k, stride, pad, Cout) of every distinct conv of torchvision's ResNet-101 at 224 x 224."""
    out = [("conv1", 224, 4, 7, 2, 3, 64)]  # NHWC4: three channels padded to four
    h, cin = 56, 64
    for layer, (mid, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), 1):
        ho = h // stride
        out += [(f"l{layer}.0.c1", h, cin, 1, 1, 0, mid), (f"l{layer}.0.c2", h, mid, 3, stride, 1, mid),
                (f"l{layer}.0.c3", ho, mid, 1, 1, 0, 4 * mid), (f"l{layer}.0.ds", h, cin, 1, stride, 0, 4 * mid),
                (f"l{layer}.1.c1", ho, 4 * mid, 1, 1, 0, mid), (f"l{layer}.1.c2", ho, mid, 3, 1, 1, mid)]
        h, cin = ho, 4 * mid
    return out


def decoder_gemms(batch):
    """(M, N, K) of the attention and baseline captioners' GEMMs: encoder 2048 channels on 14 x 14 pixels, attention /
    decoder / embedding width 512, a vocabulary that is no multiple of 4."""
    E, P, D, V = 2048, 196, 512, 9490
    return [(batch * P, D, E), (batch, D, D), (batch, 4 * D, D + E), (batch, 4 * D, D), (batch, E, D), (batch, D, E),
            (batch, V, D), (batch * 20, V, D)]


def _problem(GemmProblem, M, N, K, lda, ldb, ldc, conv=None):
    p = GemmProblem()
    p.M, p.N, p.K, p.ksplit = M, N, K, 1
    p.A, p.B, p.C = PTR["A"], PTR["B"], PTR["C"]
    p.lda, p.ldb, p.ldc = lda, ldb, ldc
    p.alpha, p.beta = 1.0, 0.0
    if conv:
        (p.cN, p.cH, p.cW, p.cCin, p.cKH, p.cKW, p.cStride, p.cPad, p.cHo, p.cWo) = conv
    return p


def base_problems(GemmProblem):
    """[(label, amode, bmode, tiles, problem)]: tiles = the tile values queried on the unmodified problem."""
    out = []
    for batch in (1, 5, 64):
        for name, h, cin, k, s, pad, cout in resnet101_convs():
            ho = (h + 2 * pad - k) // s + 1
            conv = (batch, h, h, cin, k, k, s, pad, ho, ho)
            m, kk = batch * ho * ho, k * k * cin
            out.append((f"conv b{batch} {name}", 4 if cin == 4 else 2, 0, TILES,
                        _problem(GemmProblem, m, cout, kk, 0, kk, cout, conv)))
            # dW[Cout][(kh, kw, ci)] = dY^T . im2col(X): A = dY as k rows, B = the conv input
            out.append((f"wgrad b{batch} {name}", 1, 2, TILES, _problem(GemmProblem, cout, kk, m, cout, 0, kk, conv)))
            if k == 1 and s == 1:  # a 1x1 conv's input as dense rows (x3d / x3s take the prologue there)
                out.append((f"dense1x1 b{batch} {name}", 0, 0, TILES, _problem(GemmProblem, m, cout, kk, kk, kk, cout)))
    for batch in (5, 64):
        for m, n, k in decoder_gemms(batch):
            for a, b in ((0, 0), (0, 1), (1, 1), (1, 0)):
                out.append((f"decoder b{batch} {m}x{n}x{k} a{a}b{b}", a, b, TILES,
                            _problem(GemmProblem, m, n, k, k if a == 0 else m, k if b == 0 else n, n)))
    # past the kernels' 32-bit offsets: a conv input of 2^31 bytes (2^24 output pixels as a weight gradient's k), dense
    # rows of 2^31 bytes
    conv = (64, 512, 512, 32, 3, 3, 1, 1, 512, 512)
    out.append(("range conv", 2, 0, TILES, _problem(GemmProblem, 1 << 24, 64, 288, 0, 288, 64, conv)))
    out.append(("range wgrad", 1, 2, TILES, _problem(GemmProblem, 64, 288, 1 << 24, 64, 0, 288, conv)))
    for a, b in ((0, 0), (0, 1), (1, 1), (1, 0)):
        m, n, k = (1 << 20, 512, 512) if a == 0 else (512, 512, 1 << 20)
        out.append((f"range dense a{a}b{b}", a, b, TILES,
                    _problem(GemmProblem, m, n, k, k if a == 0 else m, k if b == 0 else n, n)))
    import gemm_contract_cases as G
    for case in G.CASES + G.REFUSALS:
        for i in range(len(case.geoms)):
            L = G.layout(case, i)
            g = L.geo
            conv = (g["N"], g["H"], g["W"], g["Cin"], g["KH"], g["KW"], g["stride"], g["pad"], g["Ho"], g["Wo"]) \
                if g else None
            p = _problem(GemmProblem, L.M, L.N, L.K, L.lda, L.ldb, L.ldc, conv)
            p.a_r1, p.a_s2, p.c_r1, p.c_s2 = L.a_r1, L.a_s2, L.c_r1, L.c_s2
            p.ksplit, p.c_split_stride = L.ksplit, L.c_split_stride
            alpha, aptr, beta, relu, b1, b2 = G.epilogue(case)
            p.alpha, p.beta, p.relu = alpha, beta, int(relu)
            p.alpha_ptr = PTR["alpha_ptr"] if aptr is not None else None
            p.bias = PTR["bias"] if b1 else None
            p.bias2 = PTR["bias"] + 0x1000 if b2 else None
            p.stats = PTR["stats"] if case.stats else None
            if case.pro:
                p.in_scale, p.in_shift = PTR["in_scale"], PTR["in_shift"]
            out.append((f"contract {case.id}[{i}]", case.amode, case.bmode, (case.tile, TILE_AUTO), p))
    return out


def _set(**kw):
    def f(p):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


def _bump(field, by):
    def f(p):
        setattr(p, field, (getattr(p, field) or 0) + by)
    return f


def _ksplit2(p):
    p.ksplit, p.c_split_stride = 2, max(1, p.M) * max(1, p.ldc)


def _c_remap(p):
    p.c_r1, p.c_s2, p.ldc = 5, p.ldc, p.ldc * ((p.M + 4) // 5)


# the epilogue and addressing variants that steer a branch of the planner, applied one at a time
VARIANTS = (
    ("alpha", _set(alpha=-0.75)), ("alpha_ptr", _set(alpha_ptr=PTR["alpha_ptr"])), ("beta1", _set(beta=1.0)),
    ("bias", _set(bias=PTR["bias"])), ("relu", _set(relu=1)), ("c_r1", _c_remap), ("stats", _set(stats=PTR["stats"])),
    ("prologue", _set(in_scale=PTR["in_scale"], in_shift=PTR["in_shift"])),
    ("prologue-unpaired", _set(in_scale=PTR["in_scale"], in_shift=None)),
    ("prologue-unaligned", _set(in_scale=PTR["in_scale"] + 4, in_shift=PTR["in_shift"])),
    ("ksplit2", _ksplit2), ("A+4", _bump("A", 4)), ("B+4", _bump("B", 4)), ("C+4", _bump("C", 4)),
    ("stats+4", _set(stats=PTR["stats"] + 4)), ("lda+1", _bump("lda", 1)), ("ldb+1", _bump("ldb", 1)),
    ("ldc+1", _bump("ldc", 1)), ("ldb+4", _bump("ldb", 4)),
)


def queries(GemmProblem):
    """[(label, amode, bmode, tile, flags, problem)], the same list on every run."""
    out = []
    for label, a, b, tiles, base in base_problems(GemmProblem):
        variants = []
        for name, change in VARIANTS:
            p = GemmProblem.from_buffer_copy(base)
            change(p)
            variants.append((name, p))
        for flags in FLAGS + REFUSED_FLAGS:
            for tile in dict.fromkeys(tiles):
                out.append((f"{label} flags {flags} tile {tile}", a, b, tile, flags, base))
            for name, p in variants:
                out.append((f"{label} flags {flags} tile {TILE_AUTO} {name}", a, b, TILE_AUTO, flags, p))
    return out


def run(lib, qs):
    """int32 [len(qs), 6]: rc and the five outputs of capmi_gemm_sk_plan per query."""
    rows = np.full((len(qs), 6), -1, dtype=np.int32)
    v = (ctypes.c_int * 5)()
    ptrs = [ctypes.cast(ctypes.byref(v, 4 * i), ctypes.POINTER(ctypes.c_int)) for i in range(5)]
    plan, byref = lib.capmi_gemm_sk_plan, ctypes.byref
    for i, (_, a, b, tile, flags, p) in enumerate(qs):
        v[0] = v[1] = v[2] = v[3] = v[4] = -1
        rows[i, 0] = plan(byref(p), a, b, tile, flags, *ptrs)
        rows[i, 1:] = v[:]
    return rows


def check_not_hollow(qs, rows):
    """The conditions the table must meet to pin anything (asserted on the generating build's answers)."""
    flags = np.array([q[4] for q in qs])
    rc, bm, bn, sk, gen, nt = rows.T
    ok = rc == 0
    for f in FLAGS:
        assert (ok & (flags == f)).any() and (~ok & (flags == f)).any(), f"flags {f}: accepted and refused rows"
    for f in REFUSED_FLAGS:
        assert not (ok & (flags == f)).any(), f"flags {f} accepted"
    for code in (EINVAL, EALIGN, ERANGE):
        assert (rc == code).any(), f"no row with rc {code}"
    assert set(gen[ok & (flags == 8)]) == {16, 32}, "x3p k-tile depths"
    assert set(gen[ok & (flags == 2)]) == {1, 2, 4}, "bf16-IO stages"
    for f in (128, 129):
        assert (gen[ok & (flags == f)] > 1).any() and (gen[ok & (flags == f)] == 1).any(), "x3w k-splits"
    nt_rows = ok & np.isin(flags, (0, 1, 16))
    assert (nt_rows & (nt == 512)).any(), "the 512-thread nt form"
    assert (nt_rows & (gen == 1)).any(), "the generic fall-back"
    for f in (0, 1, 16, 4, 8, 32):
        assert set(sk[ok & (flags == f)]) == {0, 1}, f"flags {f}: stream-K on and off"


def digest(rows):
    return hashlib.sha256(np.ascontiguousarray(rows).tobytes()).hexdigest()


def main(argv):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "image-captioning-with-different-decoders_amd"))
    sys.path.insert(0, HERE)
    from capmi._lib import LIB_PATH, GemmProblem, lib
    got = lib.capmi_gemm_workspace_bytes()
    assert got == workspace_bytes(CUS), f"{LIB_PATH} plans for another CU count (workspace {got} bytes)"
    qs = queries(GemmProblem)
    rows = run(lib, qs)
    print(f"{LIB_PATH}: {len(qs)} queries, {int((rows[:, 0] == 0).sum())} accepted, sha256 {digest(rows)}")
    if "--write" in argv:
        check_not_hollow(qs, rows)
        np.savez_compressed(TABLE, rows=rows)
        print(f"wrote {TABLE} ({os.path.getsize(TABLE)} bytes)")
    if "--dump" in argv:
        np.save(argv[argv.index("--dump") + 1], rows)


if __name__ == "__main__":
    main(sys.argv[1:])
