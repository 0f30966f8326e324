"""GPU: capmi_bn_finalize with every statistics load of a thread in flight before its first add (csrc/bn_final.h:
full batches of 16 slices per lane, then one predicated batch of 16, or of 4 when at most 256 slices remain) and
the channel parameters requested at kernel entry. The canonical fp64 order is unchanged, so every output is still
the numpy restatement below BIT FOR BIT; the T values walk every path of the loop, including lanes of one wave
that take different paths, the C values a ragged last channel group and more than one workgroup."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# T: 1 a single slice; 7 fewer slices than lanes; 63 / 64 / 65 around one slice per lane; 196, 784 the layer3 and
# layer2 shapes; 255 / 256 / 257 the short (4-slot) against the full (16-slot) predicated batch; 1023 lane 63 has
# no full batch of 16 while the others do; 1024 / 1025 exactly one full batch, and one slice past it; 1100 a full
# batch plus a remainder; 1280 / 1281 a full batch plus the short / the full predicated batch; 2048 + 17 two full
# batches plus a remainder
TS = [1, 7, 63, 64, 65, 196, 255, 256, 257, 784, 1023, 1024, 1025, 1100, 1280, 1281, 2048 + 17]
CS = [8, 20, 264]


def _K():
    from capmi import kernels as K
    return K


def canonical_ref(stats, count, gamma, beta, rm, rv, momentum, eps):
    """The canonical order of csrc/bn_final.h restated: q_l = the sequential fp64 sum of slices l, l + 64, ... in
    ascending t (l = 0..63), r_w = q_8w + ... + q_8w+7 in order, total = r_0 + ... + r_7 in order (each chain
    starts from +0.0); then the finalize arithmetic, every operation rounded on its own."""
    st = stats.astype(np.float64)  # (T, C, 2)
    T, C, _ = st.shape
    q = np.zeros((64, C, 2))
    for t in range(T):  # ascending t: lane t % 64 adds its next slice
        q[t % 64] = q[t % 64] + st[t]
    tot = np.zeros((C, 2))
    for w in range(8):
        r = np.zeros((C, 2))
        for s8 in range(8):
            r = r + q[8 * w + s8]
        tot = tot + r
    n = np.float64(count)
    mean = tot[:, 0] / n
    var = tot[:, 1] / n - mean * mean
    var = np.where(var < 0, 0.0, var)
    inv = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    sc = (gamma.astype(np.float64) * inv).astype(np.float32)
    sh = (beta.astype(np.float64) - mean * sc.astype(np.float64)).astype(np.float32)
    out = {"scale": sc, "shift": sh, "mean": mean.astype(np.float32), "var": var.astype(np.float32)}
    if rm is not None:
        unb = var * n / (n - 1.0) if count > 1 else var
        m = np.float32(momentum)
        one_m = np.float32(1.0) - m
        out["running_mean"] = one_m * rm + m * mean.astype(np.float32)
        out["running_var"] = one_m * rv + m * unb.astype(np.float32)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _run(T, C, count, running=True, save=True):
    K = _K()
    g = torch.Generator().manual_seed(1000 * C + T)
    # slice sums of mixed sign over four decades (a different association changes the rounded total), sums of
    # squares large enough for a non-negative variance
    mag = torch.exp(torch.rand(T, C, generator=g) * 9.2)
    sm = (torch.randn(T, C, generator=g) * mag).float()
    sq = (sm.double() ** 2 / 64 * (1 + torch.rand(T, C, generator=g, dtype=torch.float64))).float() + 1.0
    stats = torch.stack([sm, sq], -1).contiguous()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).float(), torch.randn(C, generator=g).float()
    rm = torch.randn(C, generator=g).float() if running else None
    rv = (torch.rand(C, generator=g) + 0.5).float() if running else None
    d = lambda x: None if x is None else x.to(DEV)  # noqa: E731
    st_d, ga_d, be_d, rm_d, rv_d = d(stats), d(gamma), d(beta), d(rm), d(rv)
    scale, shift = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    mean = torch.empty(C, device=DEV) if save else None
    var = torch.empty(C, device=DEV) if save else None
    work = torch.zeros(K.bn_work_doubles(C), device=DEV, dtype=torch.float64)
    K.bn_finalize(st_d, T, C, count, ga_d, be_d, rm_d, rv_d, 0.1, 1e-5, scale, shift, work,
                  save_mean=mean, save_var=var)
    torch.cuda.synchronize()
    ref = canonical_ref(stats.numpy(), count, gamma.numpy(), beta.numpy(),
                        None if rm is None else rm.numpy(), None if rv is None else rv.numpy(), 0.1, 1e-5)
    got = {"scale": scale, "shift": shift}
    if save:
        got.update(mean=mean, var=var)
    if running:
        got.update(running_mean=rm_d, running_var=rv_d)
    for name, val in got.items():
        assert np.array_equal(_bits(val.cpu().numpy()), _bits(ref[name])), (name, T, C)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("T", TS)
def test_bn_finalize_chain_bitwise(T, C):
    """scale, shift, batch mean / var and the running statistics, as int32 bit patterns, on every loop path."""
    _run(T, C, 64 * T)


def test_bn_finalize_chain_no_running_stats():
    """running_mean / running_var = None: nothing is requested early, nothing is updated."""
    _run(1100, 20, 64 * 1100, running=False)


def test_bn_finalize_chain_no_saved_stats():
    """save_mean / save_var = None."""
    _run(257, 20, 64 * 257, save=False)


def test_bn_finalize_chain_ragged_count():
    """count != 64 T (a ragged last slice): the divisor is the count, not the slice total."""
    _run(196, 264, 64 * 195 + 13)
