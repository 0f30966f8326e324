"""GPU: the epilogue and addressing contract of include/capmi.h on every GEMM kernel form,

    C = alpha * alpha_ptr[0] * op(A).op(B) (+ bias + bias2) (+ beta*C) (relu)

stored through ldc and the c_r1 / c_s2 row remap, with `stats` the (sum, sumsq) of the stored values per 64-row
slice. The case table, the fp64 restatement and the rules are tests/gemm_contract_cases.py (checked on the CPU by
tests/test_gemm_contract_cases_cpu.py). Per case, one launch of a few hundred rows:

  result       |C - ref| <= 4e-6 * bound + 1e-6 inside the view, bound = |alpha*alpha_ptr| (|A|.|B|) + |bias| +
               |bias2| + |beta| |C0| (the bf16-operand forms against the reference of the rounded operands);
  NaN prefill  a beta = 0 launch leaves no NaN in the view (C is not read);
  canaries     the padding columns of the wider buffer, the guard row above, the rows at and past M, the rows a
               remap does not address and the gaps between k-split slabs are bit-unchanged;
  statistics   each stats[slice][col] pair against the fp64 sums of the kernel's own stored C over that slice,
               2 * 64 * 2^-24 * sum|v| + 1e-6; slices past ceil(M/64) keep their canary;
  instantiation  capmi_last_launch_name equals the instantiation the case names;
  stream-K     a second launch on the same workspace is bit-equal and leaves the flags zero (sk_check).

The last test asserts that the set of launched names equals the table's, so a planner change that reroutes a
case shows up, and prints the worst err / tol ratio per family."""
import ctypes
import time

import pytest
import torch

import gemm_contract_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAUNCHED = {}
_STATE = {}


def _K():
    from capmi import kernels as K
    return K


def _workspace():
    if "ws" not in _STATE:
        _STATE["ws"] = _K().gemm_workspace(DEV)
    return _STATE["ws"]


def _split3(t):
    K = _K()
    t = t.contiguous()
    out = torch.empty(3 * t.numel(), device=DEV, dtype=torch.bfloat16)
    K.split3_bf16(t, out)
    return out


def _device_problem(case, i, p, keep):
    """capmi_gemm_problem of problem i on the device; `keep` holds every tensor it points into."""
    K = _K()
    L = GC.layout(case, i)
    alpha, aptr, beta, relu, _, _ = GC.epilogue(case)
    d = {k: (v.to(DEV) if v is not None else None) for k, v in p.items()}
    A, B = d["A"], d["B"]
    if case.family in ("x3", "x3p", "x3d", "x3s", "x3c"):
        if case.family in ("x3p", "x3d", "x3c") and L.geo is not None:
            B = B.clone()  # the weight in the x3p conv k order (ci / 32, kh, kw, ci % 32)
            B[:, :L.K] = K.conv_weight_order_x3p(B[:, :L.K].contiguous(), L.geo["KH"], L.geo["KW"], L.geo["Cin"])
        B = _split3(B)     # three bf16 planes [3][N][ldb]
        if case.family == "x3p":
            A = _split3(A)  # dense [3][M][lda], conv [3][n*H*W][Cin]
    keep.extend([d, A, B])
    prob = K.problem(L.M, L.N, L.K, A, L.lda, B, L.ldb, d["C"][L.c_off:], L.ldc, a_r1=L.a_r1, a_s2=L.a_s2,
                     c_r1=L.c_r1, c_s2=L.c_s2, ksplit=L.ksplit, c_split_stride=L.c_split_stride, bias=d["bias"],
                     bias2=d["bias2"], alpha=alpha, alpha_ptr=d["alpha_ptr"], beta=beta, relu=relu,
                     stats=d["stats"], conv=L.geo, in_scale=d["in_scale"], in_shift=d["in_shift"])
    return L, d, prob


def _launch(case, probs):
    """The launch's return code (0, or a CAPMI_E* code)."""
    from capmi._lib import GemmProblem, lib
    K = _K()
    if case.api == "gemm":
        arr = (GemmProblem * len(probs))(*probs)
        if case.flags:
            return lib.capmi_gemm_ex(arr, len(probs), case.amode, case.bmode, case.tile, case.flags, K.stream())
        return lib.capmi_gemm(arr, len(probs), case.amode, case.bmode, case.tile, K.stream())
    ws = _workspace() if case.ws else None
    return lib.capmi_gemm_sk_ex(ctypes.byref(probs[0]), case.amode, case.bmode, case.tile, case.flags,
                                K.ptr(ws), ws.numel() * 4 if ws is not None else 0, K.stream())


def run_case(case):
    K = _K()
    inp = GC.make_inputs(case)
    ref = GC.gemm_contract_ref(case, inp)
    keep, built = [], []
    for i, p in enumerate(inp):
        built.append(_device_problem(case, i, p, keep))
    probs = [b[2] for b in built]
    assert _launch(case, probs) == 0
    torch.cuda.synchronize()
    name = K.last_launch_name()
    LAUNCHED[case.id] = name
    assert name == case.expect, f"{case.id}: launched {name}, the case pins {case.expect}"
    alpha, aptr, beta, relu, _, _ = GC.epilogue(case)
    first = []
    for i, (L, d, _) in enumerate(built):
        after = d["C"].cpu()
        stats = d["stats"].cpu() if case.stats else None
        first.append((after, stats))
        mask = GC.c_view_mask(case, i)
        GC.check_canaries(case, inp[i]["C"], after, mask)
        got = after[GC.c_offsets(L)]                      # [ksplit, M, N]
        if beta == 0.0:
            assert not bool(torch.isnan(got).any()), f"{case.id}: NaN left in the view after a beta = 0 launch"
        exp, bound = ref[i]
        for z in range(L.ksplit):
            GC.check_result(case, got[z], exp[z], bound[z])
        if L.ksplit > 1:
            GC.check_result(case, got.double().sum(0), exp.sum(0), bound.sum(0))
        if case.stats:
            GC.check_stats(case, L, got[0], stats)
    if case.sk:
        # the workspace is left reusable and the result is deterministic
        for i, (L, d, _) in enumerate(built):
            d["C"].copy_(inp[i]["C"])
            if case.stats:
                d["stats"].copy_(inp[i]["stats"])
        assert _launch(case, probs) == 0
        torch.cuda.synchronize()
        for i, (L, d, _) in enumerate(built):
            assert torch.equal(d["C"].cpu().view(torch.int32), first[i][0].view(torch.int32)), \
                f"{case.id}: second launch on the same workspace differs"
            if case.stats:
                assert torch.equal(d["stats"].cpu().view(torch.int32), first[i][1].view(torch.int32)), case.id
    if case.ws and case.api == "sk":
        K.sk_check([_workspace()])


@pytest.mark.parametrize("cid", [c.id for c in GC.CASES])
def test_contract(cid):
    _STATE.setdefault("t0", time.time())
    run_case(GC.BY_ID[cid])


@pytest.mark.parametrize("cid", [c.id for c in GC.REFUSALS])
def test_omitted_fields_are_refused(cid):
    """A field the family's documented contract omits: CAPMI_EINVAL, and nothing is launched (the last launched
    kernel is still the one before, C is bit-unchanged)."""
    K = _K()
    run_case(GC.BY_ID["nt-64x64-a0b0-dp-plain"])
    before = K.last_launch_name()
    case = next(c for c in GC.REFUSALS if c.id == cid)
    inp = GC.make_inputs(case)
    keep = []
    L, d, prob = _device_problem(case, 0, inp[0], keep)
    assert _launch(case, [prob]) == GC.EINVAL
    torch.cuda.synchronize()
    assert K.last_launch_name() == before
    assert torch.equal(d["C"].cpu().view(torch.int32), inp[0]["C"].view(torch.int32))


def test_launched_names_are_the_table():
    """Coverage roll-up: every case launched the instantiation it names (cases deselected from this run are run
    here), so the set of launched names is the table's expected set."""
    for c in GC.CASES:
        if c.id not in LAUNCHED:
            run_case(c)
    assert set(LAUNCHED.values()) == {c.expect for c in GC.CASES}
    per = {}
    for c in GC.CASES:
        per.setdefault(c.family, set()).add(LAUNCHED[c.id])
    for fam in sorted(per):
        print(f"[gemm contract] {fam}: {len(per[fam])} instantiations pinned, worst err/tol "
              f"{GC.RATIOS.get(fam, 0.0):.3g}")
    print(f"[gemm contract] {len(GC.CASES)} cases, {len(set(LAUNCHED.values()))} instantiations, "
          f"{time.time() - _STATE.get('t0', time.time()):.1f} s")
