"""GPU: self-critical training of the attention captioner on features stored once per image
(capmi.decoder_group, capmi.scst.AttentionSelfCriticalStep, models.attention.train_self_critical).

* the grouped forward against DecoderCore.forward on features replicated per row;
* the sampler's log-probabilities against the teacher-forced ones of the grouped pass;
* the step's gradients against fp64 autograd of oracle.decoder_ref.decoder_forward on the GPU's own packed
  captions: the relative L2 error of the worst parameter is at most twice that of the same loss on the existing
  DecoderCore with the features repeated n times (computed in the same test);
* real rewards end to end, graph replay equal to eager bit for bit, what the step refuses, and
  train_self_critical on a tiny synthetic set.
"""
import math
import os
import types

import pytest
import torch

import gen
from helpers import assert_close, make_decoder, rel_err, t
from oracle import decoder_ref as R
from test_gpu_scst import bound, fx, tables  # noqa: F401  (fixtures: the reward bound of tests/test_gpu_scst.py)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SMALL = (3, 2, 5, 20, 24, 16, 40, 68)             # (B, n, P, A, D, M, V, E)
LARGE = (4, 5, 49, 512, 512, 512, 8100, 2048)
LR, CLIP = 1e-4, 5.0


class Feats(torch.nn.Module):
    """A frozen 'encoder' whose images are the (B, P, E) features themselves."""

    def forward(self, x):
        return x


def _decoder(A, D, M, V, E, seed, fc_scale=1.0, end_bias=0.0, train_embedding=True):
    """An AttentionDecoder of encoder width E (the class fixes 2048: the layers that see E are rebuilt) with seeded
    weights in the reference's init distributions; returns (decoder, its fp32 parameters on the host)."""
    dec, _ = make_decoder(A, D, M, V, seed, "cpu")
    dec.encoder_dim = E
    dec.attention.enc_att = torch.nn.Linear(E, A)
    dec.decode_step = torch.nn.LSTMCell(M + E, D)
    dec.h_lin, dec.c_lin, dec.f_beta = torch.nn.Linear(E, D), torch.nn.Linear(E, D), torch.nn.Linear(D, E)
    shapes = dict(gen.decoder_param_shapes(A, D, M, V, E))
    p = {}
    for k, shape in shapes.items():
        if k.startswith("decode_step"):
            b = 1.0 / math.sqrt(D)
        elif k.startswith(("fc.", "embedding.")):
            b = 0.1
        else:
            b = 1.0 / math.sqrt(shapes[k.replace("bias", "weight")][1])
        p[k] = t(gen.uniform(seed, k, shape, -b, b))
    p["fc.weight"] = p["fc.weight"] * fc_scale
    p["fc.bias"][V - 2] += end_bias
    dec.load_state_dict(p)
    dec.fine_tune_embeddings(train_embedding)
    return dec.to(DEV).train(), p


def _feats(B, P, E, seed=5):
    return t(gen.encoder_features(seed, B, P, E).reshape(B, P, E))


def _adam(dec):
    from capmi.optim import Adam
    opt = Adam([q for q in dec.parameters() if q.requires_grad], lr=LR)
    opt.set_clip(CLIP)
    return opt


def _dummy_refs(V):
    from capmi.scst import CiderRefs
    return CiderRefs.build([[[1, 2, 3]], [[2, 3, 4]], [[3, 4, 5]], [[4, 5, 6]]], end_idx=V - 2, device=DEV)


def _step(dec, refs, V, n, baseline="mean", max_steps=5, graph=False, **kw):
    from capmi.scst import AttentionSelfCriticalStep
    return AttentionSelfCriticalStep(Feats(), dec, _adam(dec), refs, num_samples=n, baseline=baseline,
                                     max_steps=max_steps, graph=graph, start_idx=V - 3, end_idx=V - 2, pad_idx=0, **kw)


# --------------------------------------------------------------------------------------------------- forward
MEDIUM = (2, 5, 49, 64, 64, 32, 104, 256)


@pytest.mark.parametrize("shape,L,precision", [(SMALL, 6, "fp32"), ((2, 5, 49, 64, 48, 32, 100, 260), 4, "fp32"),
                                               (MEDIUM, 4, "fp32-x3")])
def test_grouped_forward_against_decoder_core(shape, L, precision):
    """Equal lengths, no dropout: the grouped pass on (B, P, E) and DecoderCore on the (B n, P, E) copy, in the
    decoder's GEMM arithmetic."""
    from capmi import decoder_fn as DF
    from capmi.decoder_group import GroupedDecoder
    B, n, P, A, D, M, V, E = shape
    dec, _ = _decoder(A, D, M, V, E, 3)
    dec.eval()
    dec.set_compute_precision(precision)
    gf = DF.gemm_flags(dec)
    assert (gf != 0) == (precision != "fp32")
    enc = _feats(B, P, E).to(DEV)
    caps = t(gen.captions(3, B * n, L, V)).to(DEV)
    p = DF.decoder_params(dec)
    preds, alphas, _ = GroupedDecoder().forward(p, enc, caps, n, gemm_flags=gf)
    want, walphas, _ = DF.CORE.forward(p, enc.repeat_interleave(n, 0).contiguous(), caps, [L - 1] * (B * n),
                                       gemm_flags=gf)
    torch.cuda.synchronize()
    assert preds.shape == want.shape == (B * n, L - 1, V) and alphas.shape == (L - 1, B * n, P)
    assert_close(preds, want, 1e-4, 1e-5, "grouped predictions")
    assert_close(alphas.transpose(0, 1), walphas, 0.0, 1e-5, "grouped alphas")


def test_rollout_and_teacher_forcing_agree():
    """the log-probability the sampler recorded for a token is the one the grouped teacher-forced pass gives it"""
    B, n, P, A, D, M, V, E = SMALL
    n, ms = 4, 12
    dec, _ = _decoder(A, D, M, V, E, 5, end_bias=2.0)
    step = _step(dec, _dummy_refs(V), V, n, max_steps=ms)
    step(_feats(B, P, E).to(DEV), [0, 1, 2], seed=3, rewards=torch.rand(B * n, device=DEV), update=False)
    torch.cuda.synchronize()
    last = step.last
    lens, lp_s = last["lens"].cpu().tolist(), last["logp"].cpu()
    lp_t, logits = last["logp_rows"].cpu(), step._sc[B].core._ws
    logits = next(iter(logits.values())).preds
    assert lp_t.shape == (B * n, ms + 1) and min(lens) >= 1
    assert any(k < ms + 1 for k in lens), "no row finished early: raise the END bias"
    tol = 2 * (1e-5 + 1e-4 * float(logits.abs().max()))
    worst = 0.0
    for r, k in enumerate(lens):  # no row is skipped
        worst = max(worst, float((lp_t[r, :k] - lp_s[:k, r]).abs().max()))
        assert bool((lp_t[r, k:] == 0).all())
    print(f"sampler logp against teacher-forced logp: max abs difference {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol, (worst, tol)


# --------------------------------------------------------------------------------------------------- gradients
def _pg_loss(preds, caps, lens, adv):
    """-sum adv logp / count over the live steps t < lens of preds (R, T, V), target caps[r][t + 1]"""
    T = preds.shape[1]
    lp = torch.log_softmax(preds, -1).gather(2, caps[:, 1:T + 1, None])[..., 0]
    live = torch.arange(T, device=preds.device)[None, :] < lens[:, None]
    return -(adv[:, None] * lp * live).sum() / lens.sum()


@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["small", "large"])
def test_step_gradients_against_fp64_autograd(shape):
    """Measured on the MI355X, relative L2 of the worst parameter gradient, grouped step / replicated DecoderCore:
    6.4e-07 / 8.9e-07 at the small shape (full_att.weight), 1.23e-05 / 1.23e-05 at the large one (enc_att.bias and
    dec_att.bias, alike in both arms)."""
    from capmi import decoder_fn as DF
    from capmi import kernels as K
    B, n, P, A, D, M, V, E = shape
    ms, R_ = 5, B * n
    T, L = ms + 1, ms + 2
    dec, p = _decoder(A, D, M, V, E, 5)
    feats = _feats(B, P, E)
    step = _step(dec, _dummy_refs(V), V, n, max_steps=ms)
    rewards = torch.rand(R_, generator=torch.Generator().manual_seed(11)) * 3
    loss = step(feats.to(DEV), list(range(B)), seed=11, rewards=rewards.to(DEV), update=False)
    torch.cuda.synchronize()
    assert step.counts["eager"] == 1 and step.opt.step_count == 0
    last = step.last
    caps, lens, adv = last["caps"].cpu(), last["lens"].cpu().long(), last["adv"].cpu()
    r64 = rewards.double().view(B, n)
    assert_close(adv, (r64 - (r64.sum(1, keepdim=True) - r64) / (n - 1)).reshape(-1), 1e-6, 1e-6, "adv")
    names = [k for k, q in dec.named_parameters() if q.requires_grad]
    assert len(names) == 19
    got = {k: q.grad.detach().clone() for k, q in dec.named_parameters() if q.requires_grad}
    # fp64 autograd on the CPU, on the GPU's own packed captions and advantages
    q64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    preds64 = R.decoder_forward(q64, feats.double().repeat_interleave(n, 0), caps, [L] * R_)[0]
    loss64 = _pg_loss(preds64, caps, lens, adv.double())
    loss64.backward()
    loss64 = loss64.detach()
    print(f"loss {float(loss):.8g} fp64 {float(loss64):.8g}")
    assert abs(float(loss) - float(loss64)) <= 1e-5 * max(1.0, abs(float(loss64)))
    # the same loss on the existing DecoderCore with the features repeated n times
    pd = DF.decoder_params(dec)
    capsd = caps.to(DEV)
    preds, _, st = DF.CORE.forward(pd, feats.to(DEV).repeat_interleave(n, 0).contiguous(), capsd, [T] * R_)
    f32 = lambda *s: torch.empty(*s, device=DEV)  # noqa: E731
    inv = (1.0 / lens.sum().float()).reshape(1).to(DEV)
    dl = f32(T * R_, V)
    K.pg_ce_fwd_bwd(preds, capsd, R_, T, L, V, 1, last["lens"], 0, last["adv"], inv, f32(R_ * T), f32(R_ * T), dl, True)
    rep = {k: torch.empty_like(pd[k]) for k in names}
    DF.CORE.backward(pd, st, rep, dl, dpred_time_major=True)
    torch.cuda.synchronize()
    worst, worst_rep = 0.0, 0.0
    zero = "attention.full_att.bias"
    for k in names:
        if k == zero:
            continue
        e, e_rep = rel_err(got[k].reshape(-1), q64[k].grad.reshape(-1)), rel_err(rep[k].reshape(-1), q64[k].grad.reshape(-1))
        print(f"{k}: grouped {e:.3g} replicated DecoderCore {e_rep:.3g}")
        worst, worst_rep = max(worst, e), max(worst_rep, e_rep)
    print(f"worst parameter: grouped {worst:.3g}, replicated {worst_rep:.3g}")
    assert worst <= 2 * worst_rep, (worst, worst_rep)
    # full_att.bias shifts every score of a softmax alike: its exact gradient, the sum of all de, is zero and has
    # no relative error. What the kernels return is the rounding residue of that sum: held to the accumulation
    # rule of tests/decoder_kernel_cases.py (``within``) on the summed |de| of the step's own backward.
    de = next(iter(step._sc[B].core._ws.values())).DE
    mag = float(de.double().abs().sum())
    assert float(q64[zero].grad.abs().max()) <= 1e-12 * mag
    print(f"{zero}: grouped {float(got[zero].abs().max()):.3g} replicated {float(rep[zero].abs().max()):.3g} of an "
          f"exact 0, sum |de| {mag:.3g}")
    for g in (got[zero], rep[zero]):
        assert float(g.abs().max()) <= 4e-6 * mag + 1e-6


def test_step_follows_the_decoders_compute_precision():
    """'fp32-x3' (the benchmark's configuration: CAPMI_GEMM_SPLIT3 on every GEMM of the grouped pass, forward and
    backward) is fp32-accurate: the same rollouts (the sampler's GEMMs are fp32 MFMA either way) and rewards give
    the fp32 step's loss within the project's 1e-5 and its gradients within 3e-5 relative L2: two fp32-accurate
    passes each stand at most 1.23e-05 from fp64 (the worst parameter of the large shape above), so at most twice
    that apart."""
    B, n, P, A, D, M, V, E = MEDIUM
    feats = _feats(B, P, E).to(DEV)
    rewards = (torch.rand(B * n, generator=torch.Generator().manual_seed(3)) * 3).to(DEV)
    out = {}
    for prec in ("fp32", "fp32-x3"):
        dec, _ = _decoder(A, D, M, V, E, 5)
        dec.set_compute_precision(prec)
        step = _step(dec, _dummy_refs(V), V, n, max_steps=4)
        loss = step(feats, [0, 1], seed=9, rewards=rewards, update=False)
        torch.cuda.synchronize()
        out[prec] = (float(loss), step.last["caps"].cpu().clone(),
                     {k: q.grad.detach().clone() for k, q in dec.named_parameters() if q.requires_grad})
    (l0, c0, g0), (l1, c1, g1) = out["fp32"], out["fp32-x3"]
    assert torch.equal(c0, c1) and abs(l0 - l1) <= 1e-5 * max(1.0, abs(l0))
    for k in g0:
        if k != "attention.full_att.bias":  # (an exact zero: no relative error)
            assert rel_err(g1[k], g0[k]) <= 3e-5, (k, rel_err(g1[k], g0[k]))


# --------------------------------------------------------------------------------------------------- end to end
E2E = dict(B=8, n=4, ms=12, fc_scale=20.0, end_bias=-1.0)


def _e2e(graph=False, baseline="mean"):
    """A peaked toy decoder whose references are its own samples under two other seeds: real, non-zero rewards"""
    from capmi.sample import BatchedSampler
    from capmi.scst import CiderRefs
    _, _, P, A, D, M, V, E = SMALL
    B, n, ms = E2E["B"], E2E["n"], E2E["ms"]
    start, end = V - 3, V - 2
    dec, _ = _decoder(A, D, M, V, E, 5, fc_scale=E2E["fc_scale"], end_bias=E2E["end_bias"], train_embedding=False)
    feats = _feats(B, P, E).to(DEV)  # (the embedding is frozen: its scatter-add is atomic, the bits depend on order)
    one = BatchedSampler(dec, 1)
    refs = [[] for _ in range(B)]
    for seed in (101, 202):
        for b, per in enumerate(one.sample(feats, start, end, max_steps=ms, seed=seed)):
            refs[b].append([w for w in per[0]["seq"] if w not in (start, end, 0)])
    table = CiderRefs.build(refs, end_idx=end, device=DEV)
    return _step(dec, table, V, n, baseline, ms, graph), dec, feats, table


@pytest.mark.parametrize("baseline", ["mean", "greedy"])
def test_end_to_end_with_real_rewards(bound, baseline):  # noqa: F811
    from capmi.scst import cider_rewards_host, hyps_from_table
    B, n, V = E2E["B"], E2E["n"], SMALL[6]
    step, dec, feats, table = _e2e(baseline=baseline)
    loss = step(feats, list(range(B)), seed=7, update=False)
    torch.cuda.synchronize()
    last, sc = step.last, step._sc[B]
    assert math.isfinite(float(loss))
    want = torch.tensor(cider_rewards_host(table, hyps_from_table(last["tokens"].cpu(), last["lens"].cpu()),
                                           [r // n for r in range(B * n)], True, V - 2), dtype=F64)
    pos = float((want > 0).double().mean())
    print(f"{baseline}: rows with reward > 0: {pos:.2f}, mean reward {float(want.mean()):.3f}, loss {float(loss):.5f}")
    assert pos >= 0.5
    err = float((last["rewards"].cpu().double() - want).abs().max())
    assert err <= bound, (err, bound)
    assert abs(float(last["reward_mean"]) - float(want.mean())) <= bound
    if baseline == "greedy":
        wantg = torch.tensor(cider_rewards_host(table, hyps_from_table(sc.gtokens.cpu(), sc.glens.cpu()), range(B),
                                                True, V - 2), dtype=F64)
        err = float((last["adv"].cpu().double() - (want.view(B, n) - wantg[:, None]).reshape(-1)).abs().max())
        assert err <= bound and abs(float(last["greedy_reward_mean"]) - float(wantg.mean())) <= bound
    before = {k: q.detach().clone() for k, q in dec.named_parameters() if q.requires_grad}
    step(feats, list(range(B)), seed=8)
    torch.cuda.synchronize()
    assert step.opt.step_count == 1
    for k, q in dec.named_parameters():
        if q.requires_grad:
            assert bool(torch.isfinite(q).all()) and not torch.equal(q, before[k]), k


def _three(graph):
    step, dec, feats, _ = _e2e(graph)
    losses = [step(feats, list(range(E2E["B"])), seed=30 + s).clone() for s in range(3)]
    torch.cuda.synchronize()
    return step, torch.cat(losses).cpu(), [q.detach().cpu() for q in dec.parameters()]


def test_graph_replay_equals_eager_bit_for_bit():
    s_e, l_e, p_e = _three(False)
    s_g, l_g, p_g = _three(True)
    assert s_e.counts == {"replay": 0, "eager": 3, "capture": 0}
    assert s_g.counts == {"replay": 2, "eager": 0, "capture": 1}, s_g.counts
    assert bool(torch.isfinite(l_e).all()) and len(set(l_e.tolist())) == 3
    assert torch.equal(l_e, l_g), (l_e, l_g)
    for a, b in zip(p_e, p_g):
        assert torch.equal(a, b)


def test_what_the_step_does_not_take():
    from capmi.scst import AttentionSelfCriticalStep
    _, _, P, A, D, M, V, E = SMALL
    dec, _ = _decoder(A, D, M, V, E, 5)
    refs, opt = _dummy_refs(V), _adam(dec)
    mk = lambda enc=Feats(), d=dec, **kw: AttentionSelfCriticalStep(enc, d, opt, refs, **kw)  # noqa: E731
    with pytest.raises(NotImplementedError):
        mk(ctx=types.SimpleNamespace(distributed=True, device=torch.device(DEV)))
    with pytest.raises(NotImplementedError):
        mk(enc=torch.nn.Linear(4, 4).to(DEV))  # a trainable encoder
    bert, _ = _decoder(A, D, M, V, E, 5)
    bert.use_bert = True
    with pytest.raises(NotImplementedError):
        mk(d=bert)
    for kw in (dict(num_samples=17), dict(num_samples=1, baseline="mean"), dict(max_steps=64), dict(baseline="best")):
        with pytest.raises(ValueError):
            mk(**kw)
    mk(num_samples=16, max_steps=63)
    mk(num_samples=1, baseline="greedy")


# --------------------------------------------------------------------------------------------------- train
class TinyAttEncoder(torch.nn.Module):
    """Stands for models.encoder.EncoderAttention: the image's 2 x 2 pooled channel means through a Linear to the
    decoder's 2048 feature channels, (B, 2, 2, 2048)."""

    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Linear(3, 2048)

    def forward(self, imgs):
        return torch.relu(self.proj(torch.nn.functional.adaptive_avg_pool2d(imgs, 2).permute(0, 2, 3, 1)))


def test_train_self_critical_on_a_tiny_synthetic_set(monkeypatch, tmp_path, capsys):
    import models.attention as MA
    import models.encoder as ME
    from capmi.scst import AttentionSelfCriticalStep
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("CAPMI_TRAIN_GRAPH", raising=False)
    monkeypatch.setattr(ME, "EncoderAttention", TinyAttEncoder)
    V, A, D, M = 30, 20, 24, 16
    torch.manual_seed(0)
    dec, _ = make_decoder(A, D, M, V, 5, "cpu")
    os.makedirs("checkpoints")
    torch.save({"epoch": 0, "metrics": {}, "encoder": TinyAttEncoder().state_dict(), "decoder": dec.state_dict(),
                "encoder_optimizer": None, "decoder_optimizer": None}, os.path.join("checkpoints", "ce_0.pth.tar"))
    args = types.SimpleNamespace(synthetic=True, synthetic_size=8, synthetic_len=7, vocab_size=V, batch_size=4,
                                 workers=0, epochs=1, print_freq=1, grad_clip=5.0, decoder_lr=1e-4,
                                 fine_tune_encoder=False, fine_tune_embedding=False, max_caption_length=-1,
                                 model_name="sc_att", model="attention", checkpoint="ce_0.pth.tar", self_critical=True,
                                 use_bert=False, sc_samples=3, sc_baseline="greedy", sc_temperature=1.0, sc_top_k=0,
                                 sc_max_len=8)
    MA.train_self_critical(torch.device("cuda"), args)
    out = capsys.readouterr().out
    assert "Reward" in out and "Greedy" in out and "Loss" in out, out
    step = MA.train_self_critical.last_step
    assert isinstance(step, AttentionSelfCriticalStep)
    assert step.counts == {"replay": 1, "eager": 0, "capture": 1}, step.counts  # two batches of four images
    ck = torch.load(os.path.join("checkpoints", "sc_att_0.pth.tar"), weights_only=True)
    assert [len(e) for e in ck["metrics"]["epoch_losses"]] == [2] and len(ck["metrics"]["epoch_rewards"][0]) == 2
    assert all(math.isfinite(x) for x in ck["metrics"]["epoch_losses"][0] + ck["metrics"]["epoch_rewards"][0])
    assert any(not torch.equal(ck["decoder"][k].cpu(), v) for k, v in dec.state_dict().items())
    args.checkpoint = None
    with pytest.raises(SystemExit):
        MA.train_self_critical(torch.device("cuda"), args)
