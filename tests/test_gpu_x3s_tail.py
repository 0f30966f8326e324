"""GPU: layer1's bottleneck tails fused into a recomputed K = 64 conv pass (gemm_x3s.hip).

The statistics pass and the tail pass run gemm_x3s_kernel's tile loop, so everything here is compared as int32 bit
patterns against the path they replace: K.gemm_x3s (stored product + statistics) followed by K.bn_add_relu."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
# rows 121: two tiles, the last ragged; 98 tiles < the grid; 539 tiles > the 512-workgroup grid (workgroups loop and
# prefetch past the end); 147 rows without the prologue
SHAPES = [(1, 11, True), (2, 56, True), (11, 56, True), (3, 7, False)]
COUT, CIN = 256, 64


def _K():
    from capmi import kernels as K
    return K


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1).float()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


class _Conv:
    """One layer1-shaped 1x1 conv problem (Cin 64 -> 256 over N x H x H pixels), its operands held on the device,
    and the storing kernel's product and statistics on it (computed once per shape, never modified)."""

    def __init__(self, N, H, pro):
        K = _K()
        self.N, self.H, self.pro, self.rows = N, H, pro, N * H * H
        self.x = rnd(self.rows, CIN, seed=31).to(DEV)
        w = (rnd(COUT, CIN, seed=32) * (2.0 / CIN) ** 0.5).to(DEV)
        self.w3 = torch.empty(3 * w.numel(), device=DEV, dtype=torch.bfloat16)
        K.split3_bf16(w, self.w3)
        self.s, self.b = (rnd(CIN, seed=33) + 1.0).to(DEV), rnd(CIN, seed=34).to(DEV)
        self.ntile = K.stat_tiles(self.rows)
        self.y = torch.full((self.rows, COUT), NAN, device=DEV)
        self.stats = torch.full((2 * self.ntile * COUT,), NAN, device=DEV)
        prob, mode = self.problem(self.y, self.stats)
        assert K.gemm_x3s_ok(prob, mode)
        K.gemm_x3s(prob, mode)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(self.y).any()) and not bool(torch.isnan(self.stats).any())

    def problem(self, C, stats):
        K = _K()
        if not self.pro:
            return K.problem(self.rows, COUT, CIN, self.x, CIN, self.w3, CIN, C, COUT, stats=stats), 0
        geo = dict(N=self.N, H=self.H, W=self.H, Cin=CIN, KH=1, KW=1, stride=1, pad=0, Ho=self.H, Wo=self.H)
        return K.problem(self.rows, COUT, CIN, self.x, 0, self.w3, CIN, C, COUT, conv=geo, stats=stats,
                         in_scale=self.s, in_shift=self.b), 2


_CONVS = {}


def conv_case(N, H, pro):
    key = (N, H, pro)
    if key not in _CONVS:
        _CONVS[key] = _Conv(N, H, pro)
    return _CONVS[key]


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("N,H,pro", SHAPES)
def test_stats_pass_bit_equal_and_stores_nothing(N, H, pro, with_c):
    K = _K()
    c = conv_case(N, H, pro)
    cbuf = torch.full((c.rows + 64, COUT), NAN, device=DEV)
    stats = torch.full_like(c.stats, NAN)
    prob, mode = c.problem(cbuf[: c.rows] if with_c else None, stats)
    K.gemm_x3s_stats(prob, mode)
    assert K.last_launch_name() == K.gemm_x3s_stats_kernel_name(prob, mode)
    torch.cuda.synchronize()
    assert same_bits(stats, c.stats)
    assert bool(torch.isnan(cbuf).all()), "the statistics pass wrote C"


@pytest.mark.parametrize("N,H,pro,res,ld", [(n, h, p, r, COUT) for (n, h, p) in SHAPES for r in (False, True)]
                         + [(1, 11, True, False, 264), (3, 7, False, True, 320)])
def test_tail_pass_bit_equal(N, H, pro, res, ld):
    """res False: out = relu(bn(acc) + other); True: out = relu(bn(other) + res_bn(acc)) -- bit for bit
    K.bn_add_relu on the stored product; `other` between NaN rows, NaN rows after `out` untouched."""
    K = _K()
    c = conv_case(N, H, pro)
    rows = c.rows
    obuf = torch.full((rows + 128, ld), NAN, device=DEV)
    other = obuf[64:64 + rows]
    other[:, :COUT] = rnd(rows, COUT, seed=41).to(DEV)
    oc = other[:, :COUT].contiguous()
    s, b = (rnd(COUT, seed=42) * 2).to(DEV), rnd(COUT, seed=43).to(DEV)  # scales of both signs
    rs, rb = (rnd(COUT, seed=44) * 2).to(DEV), rnd(COUT, seed=45).to(DEV)
    assert bool((s < 0).any()) and bool((s > 0).any()) and bool((rs < 0).any())
    ref = torch.full((rows, COUT), NAN, device=DEV)
    if res:
        K.bn_add_relu(oc, s, b, c.y, ref, rows, COUT, res_scale=rs, res_shift=rb)
    else:
        K.bn_add_relu(c.y, s, b, oc, ref, rows, COUT)
    buf = torch.full((rows + 64, COUT), NAN, device=DEV)
    prob, mode = c.problem(buf[:rows], None)
    if res:
        K.gemm_x3s_tail(prob, mode, s, b, other, ld, rs, rb)
    else:
        K.gemm_x3s_tail(prob, mode, s, b, other, ld)
    assert K.last_launch_name() == K.gemm_x3s_tail_kernel_name(prob, mode, res)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ref).any())
    assert same_bits(buf[:rows], ref)
    assert bool((ref == 0).any()) and bool((ref > 0).any())  # the ReLU clips some, not all
    assert bool(torch.isnan(buf[rows:]).all()), "the tail pass wrote past row M"
    assert bool(torch.isnan(obuf[:64]).all()) and bool(torch.isnan(obuf[64 + rows:]).all())


class _Keys:
    def __init__(self):
        self.keys = []

    def __call__(self, tag, flops, launch, key):
        launch()
        self.keys.append(key)


def _encoder(seed):
    from models.encoder import EncoderAttention
    torch.manual_seed(seed)
    enc = EncoderAttention().to(DEV)
    enc.set_compute_precision("fp32-x3")
    # running statistics away from their initial (0, 1): the eval-mode forward then applies a real BN
    g = torch.Generator().manual_seed(seed + 1)
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_((torch.rand(m.num_features, generator=g) - 0.5).to(DEV))
            m.running_var.copy_((torch.rand(m.num_features, generator=g) + 0.5).to(DEV))
    return enc


def _bn_state(enc):
    return {k: v.clone() for k, v in enc.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def _assert_state_equal(a, b):
    assert a.keys() == b.keys() and len(a) > 300
    for k in a:
        if a[k].dtype == torch.float32:
            assert same_bits(a[k], b[k]), k
        else:
            assert torch.equal(a[k], b[k]), k


def _tail_keys(keys):
    return sorted(k for k in keys if "x3s_tail" in k or "x3s_stats" in k)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("B,HW", [(2, 64), (3, 72)])
def test_encoder_forward_switch_on_equals_off(B, HW, train):
    """EncoderRunner.forward with the fused layer1 tails against the conv -> bn_add_relu path, one process: features,
    every BN's running statistics and num_batches_tracked bit-equal (layer1 rows 512, and 972: a ragged tile)."""
    from models.encoder import _ResNetView
    enc = _encoder(5)
    enc.train(train)
    imgs = rnd(B, 3, HW, HW, seed=7).to(DEV)
    state0 = {k: v.clone() for k, v in enc.state_dict().items()}
    net, runner = _ResNetView(enc.resnet), enc._runner
    got = {}
    for on in (True, False):
        enc.load_state_dict(state0)
        runner.x3s_tail = on
        runner.conv_hook = hook = _Keys()
        feats = runner.forward(net, imgs, (14, 14), train=train)
        torch.cuda.synchronize()
        runner.conv_hook = None
        got[on] = (feats.clone(), _bn_state(enc), _tail_keys(hook.keys))
    stats = ["gemm_x3s_stats_kernel<4, false>"] + ["gemm_x3s_stats_kernel<4, true>"] * 2
    tails = ["gemm_x3s_tail_kernel<4, false, true>"] + ["gemm_x3s_tail_kernel<4, true, false>"] * 2
    assert got[True][2] == ((stats if train else []) + tails) and got[False][2] == []
    assert same_bits(got[True][0], got[False][0])
    _assert_state_equal(got[True][1], got[False][1])
    if train:
        assert int(got[True][1]["resnet.1.num_batches_tracked"]) == int(state0["resnet.1.num_batches_tracked"]) + 1


def test_finetune_switch_on_equals_off():
    """ft_forward + ft_backward (layer1 frozen, layer2-4 trained) with the switch on and off: features and every
    gradient bit-equal."""
    enc = _encoder(9)
    enc.train()
    enc.fine_tune(True)
    imgs = rnd(2, 3, 64, 64, seed=11).to(DEV)
    dfeat = (rnd(2, 14, 14, 2048, seed=12) * 1e-2).to(DEV)
    state0 = {k: v.clone() for k, v in enc.state_dict().items()}
    params = [(n, q) for n, q in enc.named_parameters() if q.requires_grad]
    got = {}
    for on in (True, False):
        enc.load_state_dict(state0)
        enc._runner.x3s_tail = on
        enc._runner.conv_hook = hook = _Keys()
        grads = {id(q): torch.zeros_like(q) for _, q in params}
        with torch.no_grad():
            feats = enc.ft_forward(imgs)
            enc.ft_backward(dfeat, grads)
        torch.cuda.synchronize()
        enc._runner.conv_hook = None
        got[on] = (feats.clone(), {n: grads[id(q)] for n, q in params}, _bn_state(enc), _tail_keys(hook.keys))
    assert len(got[True][3]) == 6 and got[False][3] == []
    assert same_bits(got[True][0], got[False][0])
    assert len(params) > 200
    assert sum(bool(g.any()) for g in got[False][1].values()) > 200  # (real gradients, not untouched zeros)
    for n, _ in params:
        assert same_bits(got[True][1][n], got[False][1][n]), n
    _assert_state_equal(got[True][2], got[False][2])
