"""GPU: self-critical training of the baseline captioner (csrc/scst.hip, capmi.scst).

* capmi_cider_reward against the reference scorer's fixture (tests/golden/cider_rewards.json) and, on a larger seeded
  corpus, against capmi.scst.cider_rewards_host. The bound is measured, not chosen: the formula restated in numpy
  float32 with sequential sums (scst_cases.reward_f32) has some largest error against the fixture; the kernel, whose
  sums run in another order, gets four times that, and never less than one fp32 ulp at 10 (tests/test_gpu_sample.py's
  convention). Measured on the MI355X: restatement 8.43e-07, bound 3.37e-06; kernel 6.24e-07 over the fixture,
  8.57e-07 on the larger corpus.
* capmi_rollout_pack, capmi_scst_advantage and capmi_pg_ce_fwd_bwd against a few lines of fp64.
* BaselineSelfCriticalStep: the teacher-forced log-probabilities equal the sampler's, its gradients equal fp64
  autograd's (at most twice the error of the same loss composed from BaselineDecoderFn and torch ops), real rewards
  end to end, graph replay equal to eager bit for bit, and models.baseline.train_self_critical on a tiny set.
"""
import math
import os
import random
import types

import numpy as np
import pytest
import torch

import baseline_cases as BC
import decoder_kernel_cases as DK
import gen
import scst_cases as SC
import test_gpu_baseline_train_step as TS
from helpers import assert_close, rel_err, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# --------------------------------------------------------------------------------------------------- 1. reward
@pytest.fixture(scope="module")
def fx():
    return SC.load_fixture()


@pytest.fixture(scope="module")
def tables(fx):
    """{(case, with_end): CiderRefs on the device}"""
    from capmi.scst import CiderRefs
    return {(c, e): CiderRefs.build(SC.references(fx[c]), end_idx=fx["end_idx"] if e else None, device=DEV)
            for c in ("corpus", "single_image") for e in (False, True)}


@pytest.fixture(scope="module")
def bound(fx, tables):
    """four times the float32 restatement's largest error over all fixture rows, at least one ulp at 10"""
    end, worst = fx["end_idx"], 0.0
    for (c, with_end), refs in tables.items():
        for r in SC.case_rows(fx[c]):
            hyp = SC.emitted(r, end) if with_end else r["hyp"]
            want = r["score_end" if with_end else "score"]
            worst = max(worst, abs(SC.reward_f32(refs, hyp, r["image"]) - want))
    b = max(4 * worst, SC.ULP_AT_10)
    print(f"float32 restatement: max abs error {worst:.3e} over the fixture; kernel bound {b:.3e}")
    return b


def _rewards(refs, rows, n, T, end, score_end, V=65534):
    """the kernel on the table these rows make; lens come from capmi_rollout_pack"""
    from capmi import kernels as K
    tab, lens = SC.token_table(rows, T, end)
    R = len(rows)
    assert R % n == 0 and all(rows[r]["image"] == rows[r - r % n]["image"] for r in range(R))
    tok = _dev(tab)
    lens_d = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    caps = torch.zeros(R, T + 1, dtype=torch.int64, device=DEV)
    inv = torch.zeros(1, device=DEV)
    K.rollout_pack(tok, T, R, 1, end, 0, lens_d, caps, None, inv)
    keys = _dev([rows[b * n]["image"] for b in range(R // n)], torch.int32)
    out = torch.full((R,), float("nan"), device=DEV)
    K.cider_reward(tok, T, R, n, lens_d, keys, refs, V, end, score_end, out)
    torch.cuda.synchronize()
    assert lens_d.cpu().tolist() == lens.tolist()
    return out.cpu()


def _pick(case, B, n, T, end):
    """B groups of n fixture rows of one image each whose emitted tokens fit T steps; images repeat when B exceeds
    the corpus, with other rows"""
    by_image = {}
    for r in SC.case_rows(case):
        if len(SC.emitted(r, end)) <= T:
            by_image.setdefault(r["image"], []).append(r)
    elig = [v for _, v in sorted(by_image.items()) if len(v) >= n]
    assert elig
    rows = []
    for b in range(B):
        fit = elig[b % len(elig)]
        off = (b // len(elig)) * n + b + T
        rows.extend(fit[(off + k) % len(fit)] for k in range(n))
    return rows


def _check(got, rows, with_end, bound, what):
    want = torch.tensor([r["score_end" if with_end else "score"] for r in rows], dtype=F64)
    err = float((got.double() - want).abs().max())
    print(f"{what}: kernel max abs error {err:.3e} (bound {bound:.3e}), {int((want == 0).sum())} zero rows")
    assert err <= bound, (what, err, bound)
    assert bool((got[want == 0] == 0).all()), f"{what}: a golden 0 came out non-zero"
    return err


@pytest.mark.parametrize("with_end", [False, True])
@pytest.mark.parametrize("T", [1, 12, 64])
@pytest.mark.parametrize("B,n", [(1, 1), (1, 3), (3, 1), (3, 3), (40, 1), (40, 3)])
def test_reward_matches_the_fixture(fx, tables, bound, B, n, T, with_end):
    end = fx["end_idx"]
    rows = _pick(fx["corpus"], B, n, T, end)
    got = _rewards(tables[("corpus", with_end)], rows, n, T, end, with_end)
    _check(got, rows, with_end, bound, f"B {B} n {n} T {T} end {with_end}")


@pytest.mark.parametrize("with_end", [False, True])
def test_reward_on_every_fixture_row_and_alone(fx, tables, bound, with_end):
    """all rows of both corpora at T = 64; a row scores the same alone as inside its batch, bit for bit"""
    end, worst = fx["end_idx"], 0.0
    for c in ("corpus", "single_image"):
        rows = SC.case_rows(fx[c])  # 9 rows per image, image-major
        got = _rewards(tables[(c, with_end)], rows, 3, 64, end, with_end)
        worst = max(worst, _check(got, rows, with_end, bound, f"{c} end {with_end}"))
        for r in range(0, len(rows), 5):
            alone = _rewards(tables[(c, with_end)], rows[r:r + 1], 1, 64, end, with_end)
            assert alone[0].view(torch.int32) == got[r].view(torch.int32), (c, r, float(alone[0]), float(got[r]))
    print(f"kernel max abs error over every fixture row, end {with_end}: {worst:.3e}")


def test_reward_on_a_larger_corpus_against_the_host_oracle(bound):
    from capmi.scst import CiderRefs, cider_rewards_host
    rng = random.Random(77)
    end, B, n, T = 61, 64, 5, 24
    corpus = [[[rng.randint(2, 60) for _ in range(rng.randint(4, 18))] for _ in range(rng.randint(1, 6))]
              for _ in range(200)]
    refs = CiderRefs.build(corpus, end_idx=end, device=DEV)
    rows = []
    for b in range(B):
        image = rng.randrange(200)
        for _ in range(n):
            base = rng.choice(corpus[image])
            hyp = [w if rng.random() < 0.7 else rng.randint(2, 60) for w in base if rng.random() < 0.9][:T - 1]
            rows.append(dict(image=image, hyp=hyp, finished=rng.random() < 0.8))
    for score_end in (True, False):
        got = _rewards(refs, rows, n, T, end, score_end, V=62)
        want = cider_rewards_host(refs, [SC.emitted(r, end) for r in rows], [r["image"] for r in rows], score_end, end)
        err = float((got.double() - torch.tensor(want, dtype=F64)).abs().max())
        print(f"larger corpus, score_end {score_end}: max abs error {err:.3e}, mean reward {np.mean(want):.3f}")
        assert np.mean(np.array(want) > 0) > 0.5
        assert err <= bound, (err, bound)


def test_reward_of_an_unknown_image_key_is_nan(fx, tables):
    from capmi import kernels as K
    tok = torch.full((4, 2), 3, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, device=DEV)
    K.cider_reward(tok, 4, 2, 1, _dev([4, 4], torch.int32), _dev([0, 10 ** 6], torch.int32),
                   tables[("corpus", False)], 100, fx["end_idx"], True, out)
    got = out.cpu()
    assert math.isfinite(float(got[0])) and math.isnan(float(got[1]))


# --------------------------------------------------------------------------------------------------- 2. pack
def test_rollout_pack():
    from capmi import kernels as K
    start, end, pad, T = 9, 2, 0, 5
    tab = np.array([[2, -1, -1, -1, -1],      # END at step 0
                    [4, 5, 6, 7, 8],          # END never emitted
                    [4, 5, 0, -1, -1],        # the loop stopped early: -1 without END (a sampled PAD stays)
                    [4, 2, -1, -1, -1],       # finished at step 1
                    [-1, -1, -1, -1, -1],     # nothing emitted
                    [3, 2, 7, 7, 7]],         # whatever follows END is not part of the caption
                   dtype=np.int32).T.copy()   # (T, R)
    R = tab.shape[1]
    want_caps, want_lens = [], []
    for r in range(R):
        col, n = tab[:, r].tolist(), 0
        while n < T and col[n] >= 0:
            n += 1
            if col[n - 1] == end:
                break
        want_lens.append(n)
        want_caps.append([start] + col[:n] + [pad] * (T - n))
    lens = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    caps = torch.full((R, T + 1), -1, dtype=torch.int64, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    inv = torch.zeros(1, device=DEV)
    K.rollout_pack(_dev(tab), T, R, start, end, pad, lens, caps, count, inv)
    torch.cuda.synchronize()
    assert want_lens == [1, 5, 3, 2, 0, 2]
    assert lens.cpu().tolist() == want_lens and caps.cpu().tolist() == want_caps
    assert int(count) == sum(want_lens) and float(inv) == float(np.float32(1) / np.float32(sum(want_lens)))
    # more rows than the workgroup has threads
    R2 = 1500
    big = np.random.default_rng(3).integers(-1, 6, size=(7, R2)).astype(np.int32)
    lens2 = torch.zeros(R2, dtype=torch.int32, device=DEV)
    caps2 = torch.zeros(R2, 8, dtype=torch.int64, device=DEV)
    K.rollout_pack(_dev(big), 7, R2, start, end, pad, lens2, caps2, count, inv)
    want2 = []
    for r in range(R2):
        col, n = big[:, r].tolist(), 0
        while n < 7 and col[n] >= 0:
            n += 1
            if col[n - 1] == end:
                break
        want2.append(n)
    assert lens2.cpu().tolist() == want2 and int(count) == sum(want2)


# --------------------------------------------------------------------------------------------------- 3. advantage
@pytest.mark.parametrize("mode", ["mean", "greedy"])
@pytest.mark.parametrize("n", [2, 5])
def test_advantage(mode, n):
    from capmi import kernels as K
    from capmi._lib import CAPMI_SCST_GREEDY, CAPMI_SCST_MEAN
    B = 7
    g = torch.Generator().manual_seed(n)
    reward = torch.rand(B, n, generator=g) * 3
    greedy = torch.rand(B, generator=g) * 3
    adv = torch.zeros(B * n, device=DEV)
    stats = torch.full((2,), float("nan"), device=DEV)
    K.scst_advantage(reward.to(DEV), greedy.to(DEV) if mode == "greedy" else None, B, n,
                     CAPMI_SCST_GREEDY if mode == "greedy" else CAPMI_SCST_MEAN, adv, stats)
    r64 = reward.double()
    want = r64 - greedy.double()[:, None] if mode == "greedy" else r64 - (r64.sum(1, keepdim=True) - r64) / (n - 1)
    assert_close(adv.view(B, n), want, 1e-6, 1e-6, f"adv {mode} n {n}")
    assert_close(stats[0], r64.mean(), 1e-6, 1e-6, "mean reward")
    assert_close(stats[1], greedy.double().mean() if mode == "greedy" else torch.zeros((), dtype=F64), 1e-6, 1e-6,
                 "mean greedy reward")


def test_advantage_mean_needs_two_samples():
    from capmi import CapmiError
    from capmi import kernels as K
    from capmi._lib import CAPMI_SCST_MEAN
    z = torch.zeros(4, device=DEV)
    with pytest.raises(CapmiError):
        K.scst_advantage(z, None, 4, 1, CAPMI_SCST_MEAN, z.clone(), z.clone())


# --------------------------------------------------------------------------------------------------- 4. weighted CE
PG_B, PG_T, PG_L = 4, 5, 7
PG_LENS = [0, PG_T, 2, 3]
PG_ADV = [1.3, -0.7, 0.0, 2.1]


@pytest.mark.parametrize("tm", [0, 1])
@pytest.mark.parametrize("tgt_off,t_first", [(0, 1), (1, 0)])
@pytest.mark.parametrize("V", [37, 1000, 8100])
def test_pg_ce_against_fp64(V, tgt_off, t_first, tm):
    """decoder_kernel_cases.ce_compare's budget (what tests/test_gpu_baseline_train_kernels.py gives the unweighted
    kernel), every magnitude scaled by |adv|; rows that are not live are exactly zero"""
    from capmi import kernels as K
    B, T, L = PG_B, PG_T, PG_L
    case = (V, tgt_off, t_first, tm)
    g = DK.gen("pg_ce", case)
    x = DK._u(g, (B, T, V), 4.0)
    caps = torch.randint(0, V, (B, L), generator=g)
    caps[1, 1 + tgt_off], caps[3, 2 + tgt_off] = 0, V - 1
    lens, adv = torch.tensor(PG_LENS, dtype=torch.int32), torch.tensor(PG_ADV)
    inv = torch.tensor([1.0 / 7.0])
    logp, loss = torch.full((B * T,), DK.NAN, device=DEV), torch.full((B * T,), DK.NAN, device=DEV)
    dl = torch.full((B * T, V), DK.NAN, device=DEV)
    K.pg_ce_fwd_bwd(x.to(DEV), caps.to(DEV), B, T, L, V, tgt_off, lens.to(DEV), t_first, adv.to(DEV), inv.to(DEV),
                    logp, loss, dl, bool(tm))
    torch.cuda.synchronize()
    x64, a64 = x.double(), adv.double()[:, None]
    tgt = caps[:, tgt_off:tgt_off + T]
    tt = torch.arange(T)[None, :]
    live = (tt >= t_first) & (tt < t_first + lens[:, None])
    assert live.sum() == sum(min(n, T - t_first) for n in PG_LENS) and live[1].sum() == T - t_first
    lse = torch.logsumexp(x64, -1)
    xt = x64.gather(2, tgt[..., None])[..., 0]
    lp = (xt - lse) * live
    mag = (lse.abs() + xt.abs())
    what = f"pg_ce V {V} off {tgt_off} first {t_first} tm {tm}"
    got_lp, got_loss = logp.cpu().view(B, T), loss.cpu().view(B, T)
    DK.within(got_lp, lp, mag, f"{what} logp_rows")
    DK.within(got_loss, -a64 * lp, mag * a64.abs(), f"{what} loss_rows")
    DK.all_zero(got_lp[~live], f"{what} logp of rows that are not live")
    DK.all_zero(got_loss[~live], f"{what} loss of rows that are not live")
    prob = torch.exp(x64 - lse[..., None])
    onehot = torch.zeros_like(x64).scatter_(2, tgt[..., None], 1.0)
    gsc = a64[..., None] * float(inv.double())
    want = (prob - onehot) * gsc * live[..., None]
    mag_dl = (prob + onehot) * gsc.abs()
    got_dl = dl.cpu().view(T, B, V).transpose(0, 1) if tm else dl.cpu().view(B, T, V)
    k = DK.ce_k(V, float(lse.abs().max()), float((x64 - lse[..., None]).abs().max()))
    rows = live & (adv != 0)[:, None]
    DK.roundings(got_dl[rows], want[rows], mag_dl[rows], k, f"{what} dlogits")
    DK.all_zero(got_dl[~rows], f"{what} dlogits of rows that are not live or carry no advantage")
    # without dlogits: the same rows
    logp2, loss2 = torch.zeros(B * T, device=DEV), torch.zeros(B * T, device=DEV)
    K.pg_ce_fwd_bwd(x.to(DEV), caps.to(DEV), B, T, L, V, tgt_off, lens.to(DEV), t_first, adv.to(DEV), None, logp2,
                    loss2, None, bool(tm))
    assert torch.equal(logp2, logp) and torch.equal(loss2, loss)


# --------------------------------------------------------------------------------------------------- the step
def _dummy_refs(V):
    from capmi.scst import CiderRefs
    return CiderRefs.build([[[1, 2, 3]], [[2, 3, 4]], [[3, 4, 5]]], end_idx=V - 2, device=DEV)


def _step(dec, refs, V, n, baseline="mean", max_steps=12, graph=False):
    from capmi.scst import BaselineSelfCriticalStep
    return BaselineSelfCriticalStep(TS.Identity(), dec, TS._adam(dec), refs, num_samples=n, baseline=baseline,
                                    max_steps=max_steps, graph=graph, start_idx=V - 3, end_idx=V - 2, pad_idx=0)


def test_sample_device_is_sample_without_the_host_copy():
    from capmi.sample import BaselineBatchedSampler
    M, H, V, B, n = 16, 24, 40, 3, 4
    dec, _ = BC.decoder(M, H, V, 5, DEV, end_bias=2.0, end_idx=V - 2)
    feats = t(gen.uniform(5, "feats", (B, M), -1, 1)).to(DEV)
    s = BaselineBatchedSampler(dec, n)
    out = s.sample(feats, V - 3, V - 2, max_steps=12, seed=3)
    tokens, logp, alive, steps = s.sample_device(feats, V - 3, V - 2, max_steps=12, seed=3)
    assert tokens.shape == (13, B * n) and tokens.dtype == torch.int32 and tokens.is_cuda and steps <= 13
    tok, lp = tokens.t().cpu().tolist(), logp.t().cpu().tolist()
    for r in range(B * n):
        d = out[r // n][r % n]
        words = d["seq"][1:] if d["finished"] else d["seq"]
        assert tok[r][:len(words)] == words and lp[r][:len(words)] == d["token_logp"]
        assert all(w == -1 for w in tok[r][len(words):])
        assert int(alive[r]) == (0 if d["finished"] else 1)


def test_rollout_and_teacher_forcing_agree():
    """the log-probability the sampler recorded for a token is the one the teacher-forced pass gives it"""
    M, H, V, B, n, ms = 16, 24, 40, 3, 4, 12
    dec, _ = BC.decoder(M, H, V, 5, DEV, end_bias=2.0, end_idx=V - 2)
    feats = t(gen.uniform(5, "feats", (B, M), -1, 1)).to(DEV)
    step = _step(dec, _dummy_refs(V), V, n)
    step(feats, [0, 1, 2], seed=3, rewards=torch.rand(B * n, device=DEV), update=False)
    torch.cuda.synchronize()
    last = step.last
    lens, lp_s = last["lens"].cpu().tolist(), last["logp"].cpu()
    lp_t, logits = last["logp_rows"].cpu(), step._sc[B].ws.logits
    assert lp_t.shape == (B * n, ms + 2) and min(lens) >= 1
    assert any(k < ms + 1 for k in lens), "no row finished early: raise the END bias"
    tol = 2 * (1e-5 + 1e-4 * float(logits.abs().max()))
    worst = 0.0
    for r, k in enumerate(lens):  # no row is skipped
        d = (lp_t[r, 1:1 + k] - lp_s[:k, r]).abs().max()
        worst = max(worst, float(d))
        assert bool((lp_t[r, 1 + k:] == 0).all()) and float(lp_t[r, 0]) == 0
    print(f"sampler logp against teacher-forced logp: max abs difference {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol, (worst, tol)


def _adv64(rewards, greedy_rewards, B, n, baseline):
    r = rewards.double().cpu().view(B, n)
    if baseline == "greedy":
        return (r - greedy_rewards.double().cpu()[:, None]).reshape(-1)
    return (r - (r.sum(1, keepdim=True) - r) / (n - 1)).reshape(-1)


def _pg_loss(logits, caps, lens, adv):
    """-sum adv logp / count over the live rows 1 <= t < 1 + lens of logits (R, L, V), target caps[r][t]"""
    R, L, _ = logits.shape
    lp = torch.log_softmax(logits, -1).gather(2, caps[..., None])[..., 0]
    tt = torch.arange(L, device=logits.device)[None, :]
    live = (tt >= 1) & (tt < 1 + lens[:, None])
    return -(adv[:, None] * lp * live).sum() / lens.sum()


@pytest.mark.parametrize("baseline", ["mean", "greedy"])
@pytest.mark.parametrize("B,n,M,H,V", [(3, 4, 16, 24, 40), (2, 2, 512, 512, 8100)])
def test_step_gradients_against_fp64_autograd(B, n, M, H, V, baseline):
    """Measured on the MI355X, relative L2 of the worst parameter gradient, step / BaselineDecoderFn composition:
    3.5e-07 / 3.3e-07 at (16, 24, 40), 6.5e-07 / 1.06e-06 at (512, 512, 8100)."""
    ms, R = 12, B * n
    dec, p, feats = TS._decoder(B, ms + 2, M, H, V, 5, DEV)
    step = _step(dec, _dummy_refs(V), V, n, baseline)
    g = torch.Generator().manual_seed(11)
    rewards, greedy_rewards = torch.rand(R, generator=g) * 3, torch.rand(B, generator=g) * 3
    loss = step(feats.to(DEV), list(range(B)), seed=11, rewards=rewards.to(DEV),
                greedy_rewards=greedy_rewards.to(DEV) if baseline == "greedy" else None, update=False)
    torch.cuda.synchronize()
    assert step.counts["eager"] == 1 and step.opt.step_count == 0
    last = step.last
    caps, lens, adv = last["caps"].cpu(), last["lens"].cpu().long(), last["adv"].cpu()
    want_adv = _adv64(rewards, greedy_rewards, B, n, baseline)
    assert_close(adv, want_adv, 1e-6, 1e-6, "adv")
    assert float((adv.abs() > 1e-3).float().mean()) >= 0.5, "the advantages test nothing"
    got = {k: q.grad.detach().clone() for k, q in dec.named_parameters()}
    # fp64 on the CPU, on the GPU's own packed captions and advantages
    q64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    f64 = feats.double().repeat_interleave(n, 0)
    loss64 = _pg_loss(TS._forward64(q64, f64, caps), caps, lens, adv.double())
    loss64.backward()
    loss64 = loss64.detach()
    print(f"loss {float(loss):.8g} fp64 {float(loss64):.8g}")
    assert TS._close(float(loss), float(loss64)), (float(loss), float(loss64))
    # the same loss from BaselineDecoderFn, torch ops and autograd on the GPU
    dec_fn, _, _ = TS._decoder(B, ms + 2, M, H, V, 5, DEV)
    capsd = caps.to(DEV)
    _pg_loss(dec_fn(feats.to(DEV).repeat_interleave(n, 0), capsd), capsd, lens.to(DEV), adv.to(DEV)).backward()
    torch.cuda.synchronize()
    fn = {k: q.grad for k, q in dec_fn.named_parameters()}
    for k in TS.NAMES:
        e, e_fn = rel_err(got[k], q64[k].grad), rel_err(fn[k], q64[k].grad)
        print(f"{k}: step {e:.3g} BaselineDecoderFn composition {e_fn:.3g}")
        assert e <= 2 * e_fn, (k, e, e_fn)


E2E = dict(M=16, H=24, V=40, B=8, n=4, ms=12, fc_scale=20.0, end_bias=-1.0)


def _e2e(graph=False, baseline="mean"):
    """A peaked toy decoder whose references are its own samples under two other seeds: real, non-zero rewards"""
    from capmi.sample import BaselineBatchedSampler
    from capmi.scst import CiderRefs
    M, H, V, B, n, ms = (E2E[k] for k in ("M", "H", "V", "B", "n", "ms"))
    start, end = V - 3, V - 2
    dec, _ = BC.decoder(M, H, V, 5, DEV, fc_scale=E2E["fc_scale"], end_bias=E2E["end_bias"], end_idx=end)
    dec.fine_tune_embeddings(False)  # its scatter-add is atomic: the bits would depend on the order
    feats = t(gen.uniform(5, "feats", (B, M), -1, 1)).to(DEV)
    one = BaselineBatchedSampler(dec, 1)
    refs = [[] for _ in range(B)]
    for seed in (101, 202):
        for b, per in enumerate(one.sample(feats, start, end, max_steps=ms, seed=seed)):
            refs[b].append([w for w in per[0]["seq"] if w not in (start, end, 0)])
    table = CiderRefs.build(refs, end_idx=end, device=DEV)
    return _step(dec, table, V, n, baseline, ms, graph), dec, feats, table


def test_end_to_end_with_real_rewards(bound):
    from capmi.scst import cider_rewards_host, hyps_from_table
    B, n, V = E2E["B"], E2E["n"], E2E["V"]
    step, dec, feats, table = _e2e()
    keys = list(range(B))
    runs = []
    for _ in range(2):  # the same seed twice: the same bits
        loss = step(feats, keys, seed=7, update=False)
        torch.cuda.synchronize()
        runs.append((step.last["tokens"].cpu().clone(), step.last["rewards"].cpu().clone(), loss.cpu().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    last = step.last
    hyps = hyps_from_table(last["tokens"].cpu(), last["lens"].cpu())
    want = torch.tensor(cider_rewards_host(table, hyps, [r // n for r in range(B * n)], True, V - 2), dtype=F64)
    pos = float((want > 0).double().mean())
    differ = sum(len(set(want.view(B, n)[b].tolist())) > 1 for b in range(B)) / B
    print(f"rows with reward > 0: {pos:.2f}; images whose samples differ in reward: {differ:.2f}; "
          f"mean reward {float(want.mean()):.3f}")
    assert pos >= 0.5 and differ >= 0.25
    err = float((last["rewards"].cpu().double() - want).abs().max())
    assert err <= bound, (err, bound)
    err_adv = float((last["adv"].cpu().double() - _adv64(want, None, B, n, "mean")).abs().max())
    print(f"reward max abs error {err:.3e}, advantage {err_adv:.3e} (bound {bound:.3e})")
    assert err_adv <= bound, (err_adv, bound)
    assert_close(last["reward_mean"], want.mean(), 1e-6, 1e-6, "reward_mean")
    before = {k: q.detach().clone() for k, q in dec.named_parameters() if q.requires_grad}
    for s in range(3):
        step(feats, keys, seed=20 + s)
    torch.cuda.synchronize()
    assert step.opt.step_count == 3
    for k, q in dec.named_parameters():
        if q.requires_grad:
            assert bool(torch.isfinite(q).all()) and not torch.equal(q, before[k]), k


def test_greedy_baseline_with_real_rewards(bound):
    from capmi.scst import cider_rewards_host, hyps_from_table
    B, n, V = E2E["B"], E2E["n"], E2E["V"]
    step, dec, feats, table = _e2e(baseline="greedy")
    step(feats, list(range(B)), seed=7, update=False)
    torch.cuda.synchronize()
    last, sc = step.last, step._sc[B]
    want = torch.tensor(cider_rewards_host(table, hyps_from_table(last["tokens"].cpu(), last["lens"].cpu()),
                                           [r // n for r in range(B * n)], True, V - 2), dtype=F64)
    wantg = torch.tensor(cider_rewards_host(table, hyps_from_table(sc.gtokens.cpu(), sc.glens.cpu()), range(B), True,
                                            V - 2), dtype=F64)
    err = float((last["adv"].cpu().double() - (want.view(B, n) - wantg[:, None]).reshape(-1)).abs().max())
    print(f"greedy baseline: advantage max abs error {err:.3e}, mean greedy reward {float(wantg.mean()):.3f}")
    assert err <= bound
    assert_close(last["greedy_reward_mean"], wantg.mean(), 1e-6, 1e-6, "greedy_reward_mean")


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
    from capmi.optim import Adam
    from capmi.scst import BaselineSelfCriticalStep
    dec, _ = BC.decoder(16, 24, 40, 5, DEV)
    refs, opt = _dummy_refs(40), TS._adam(dec)
    with pytest.raises(NotImplementedError):
        BaselineSelfCriticalStep(TS.Identity(), dec, opt, refs, encoder_optimizer=Adam([torch.nn.Parameter(
            torch.zeros(4, device=DEV))], lr=1e-4))
    with pytest.raises(ValueError):
        BaselineSelfCriticalStep(TS.Identity(), dec, opt, refs, num_samples=1, baseline="mean")
    with pytest.raises(ValueError):
        BaselineSelfCriticalStep(TS.Identity(), dec, opt, refs, max_steps=64)


# --------------------------------------------------------------------------------------------------- train
def test_train_self_critical_on_a_tiny_synthetic_set(monkeypatch, tmp_path, capsys):
    import models.baseline as MB
    from capmi.scst import BaselineSelfCriticalStep
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("CAPMI_TRAIN_GRAPH", raising=False)
    monkeypatch.setattr(MB, "Encoder", TS.TinyEncoder)
    V, M, H = 30, 16, 24
    torch.manual_seed(0)
    dec = MB.BaselineDecoder(TS._params(V, M, H))
    os.makedirs("checkpoints")
    torch.save({"epoch": 0, "metrics": {}, "encoder": TS.TinyEncoder(M).state_dict(), "decoder": dec.state_dict(),
                "encoder_optimizer": None, "decoder_optimizer": None}, os.path.join("checkpoints", "ce_0.pth.tar"))
    args = types.SimpleNamespace(synthetic=True, synthetic_size=8, synthetic_len=7, vocab_size=V, batch_size=4,
                                 workers=0, epochs=1, print_freq=1, grad_clip=5.0, decoder_lr=1e-4,
                                 fine_tune_encoder=False, fine_tune_embedding=False, max_caption_length=-1,
                                 model_name="sc", model="baseline", checkpoint="ce_0.pth.tar", self_critical=True,
                                 sc_samples=3, sc_baseline="greedy", sc_temperature=1.0, sc_top_k=0, sc_max_len=8)
    MB.train_self_critical(torch.device("cuda"), args)
    out = capsys.readouterr().out
    assert "Reward" in out and "Greedy" in out and "Loss" in out, out
    step = MB.train_self_critical.last_step
    assert isinstance(step, BaselineSelfCriticalStep)
    assert step.counts == {"replay": 1, "eager": 0, "capture": 1}, step.counts  # two batches of four images
    ck = torch.load(os.path.join("checkpoints", "sc_0.pth.tar"), weights_only=True)
    assert [len(e) for e in ck["metrics"]["epoch_losses"]] == [2] and len(ck["metrics"]["epoch_rewards"][0]) == 2
    assert all(math.isfinite(x) for x in ck["metrics"]["epoch_losses"][0] + ck["metrics"]["epoch_rewards"][0])
    assert any(not torch.equal(ck["decoder"][k].cpu(), v) for k, v in dec.state_dict().items())
    args.checkpoint = None
    with pytest.raises(SystemExit):
        MB.train_self_critical(torch.device("cuda"), args)
