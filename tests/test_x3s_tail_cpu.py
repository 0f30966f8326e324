"""CPU: capmi_gemm_x3s_stats / capmi_gemm_x3s_tail validate on the host and refuse malformed calls before any
launch (no GPU needed: every call here must fail in the argument checks; the pointers are never dereferenced)."""
import ctypes

import pytest

EINVAL, EALIGN = 1001, 1002
A, B, C, ST, S, SH, O, RS, RB = (0x10000 * (i + 1) for i in range(9))  # fake, 16-B aligned device addresses


def _lib():
    from capmi._lib import lib
    return lib


def _prob(M=200, N=256, K=64):
    from capmi._lib import GemmProblem
    p = GemmProblem()
    p.M, p.N, p.K, p.ksplit = M, N, K, 1
    p.A, p.lda, p.B, p.ldb, p.C, p.ldc = A, K, B, K, C, N
    p.alpha, p.beta, p.stats = 1.0, 0.0, ST
    return p


def _tail(p, scale=S, shift=SH, other=O, ld=256, rs=None, rb=None, res=0, amode=0):
    return _lib().capmi_gemm_x3s_tail(ctypes.byref(p) if p is not None else None, amode, scale, shift, other, ld,
                                      rs, rb, res, None)


def test_stats_rejects_null_and_shapes():
    lib = _lib()
    assert lib.capmi_gemm_x3s_stats(None, 0, None) == EINVAL
    for field in ("A", "B", "stats"):
        p = _prob()
        setattr(p, field, None)
        assert lib.capmi_gemm_x3s_stats(ctypes.byref(p), 0, None) == EINVAL, field
    assert lib.capmi_gemm_x3s_stats(ctypes.byref(_prob(N=512)), 0, None) == EINVAL
    assert lib.capmi_gemm_x3s_stats(ctypes.byref(_prob(K=128)), 0, None) == EINVAL
    # N = 64 / 128 are x3s shapes, but only N = 256 has the two passes
    assert lib.capmi_gemm_x3s_stats(ctypes.byref(_prob(N=128)), 0, None) == EINVAL


def test_tail_rejects_null_pointers():
    assert _tail(None) == EINVAL
    assert _tail(_prob(), scale=None) == EINVAL
    assert _tail(_prob(), shift=None) == EINVAL
    assert _tail(_prob(), other=None) == EINVAL
    for field in ("A", "B", "C"):
        p = _prob()
        setattr(p, field, None)
        assert _tail(p) == EINVAL, field


@pytest.mark.parametrize("kw", [dict(N=512), dict(K=128), dict(N=128)])
def test_tail_rejects_shapes(kw):
    assert _tail(_prob(**kw)) == EINVAL
    assert _tail(_prob(**kw), rs=RS, rb=RB, res=1) == EINVAL


def test_tail_rejects_wrong_scale_shift_pairing():
    # accumulator = main branch: no residual-side BN
    assert _tail(_prob(), rs=RS, rb=RB, res=0) == EINVAL
    assert _tail(_prob(), rs=RS, res=0) == EINVAL
    # accumulator = residual branch: both of its scale and shift
    assert _tail(_prob(), res=1) == EINVAL
    assert _tail(_prob(), rs=RS, res=1) == EINVAL
    assert _tail(_prob(), rb=RB, res=1) == EINVAL
    assert _tail(_prob(), res=2, rs=RS, rb=RB) == EINVAL


def test_tail_rejects_other_layout():
    assert _tail(_prob(), other=O + 4) == EALIGN
    assert _tail(_prob(), other=O + 4, rs=RS, rb=RB, res=1) == EALIGN
    assert _tail(_prob(), ld=255) == EINVAL  # ld_other < N
    assert _tail(_prob(M=1 << 20), ld=1 << 10) == EINVAL  # M * ld_other * 4 >= 2^31
