"""GPU: the caption metrics on the device (csrc/score.hip, capmi.devscore) and the mixed self-critical reward.

* capmi_caption_stats on the seeded tables of tests/score_cases.py: the integers equal the oracle's exactly; bleu and
  rouge lie within one fp32 ulp of the fp64 oracle's value rounded to fp32 (the few scalars of a row are computed in
  fp64 on the device and rounded once: only the device's fp64 exp / cbrt / sqrt differ); a ROUGE-L of 0 is exactly 0;
  a row scores the same bits alone as inside its batch, and run to run.
* caption_scores_device on tests/golden/caption_scores.json: BLEU-1..4 and ROUGE-L come from the device's integers
  through the host's fp64 formulas, 1e-9 relative; CIDEr is capmi_cider_reward on a table of this corpus, under the
  bound rule of tests/test_gpu_scst.py (four times the float32 restatement's largest error on these rows, at least
  one fp32 ulp at 10).
* capmi_reward_mix within one fp32 ulp of the fp64 combination of its own inputs.
* Both self-critical steps with ``reward_mix``: rewards against the oracle's components, graph replay equal to eager
  bit for bit, and ``reward_mix=None`` equal bit for bit to a step built without the keyword.
* Both ``evaluate_batched`` with ``args.scorer = "device"`` against ``"host"``, and
  ``models.baseline.train_self_critical`` with ``args.sc_reward_mix`` on a tiny set.

Measured on the MI355X: bleu and rouge equal the rounded oracle on every row of every case (0 ulp); fixture CIDEr
off by 5e-08 (corpus, bound 2.4e-06) and 6e-08 (single image, bound 9.5e-07); mixed rewards off by at most 1.3e-07
(baseline) and 6.5e-08 (attention) against a least bound of 3.4e-06.
"""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import baseline_cases as BC
import eval_cases as EC
import gen
import scst_cases as SC
import score_cases as S
import test_gpu_baseline_train_step as TS
import test_gpu_scst_attention as TA
from helpers import make_decoder, t
from test_gpu_scst import bound, fx, tables  # noqa: F401  (fixtures: the reward bound of tests/test_gpu_scst.py)

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
MIX = dict(cider=1.0, bleu4=0.5, rouge_l=0.25)
WEIGHTS = (1.0, 0.5, 0.25)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@pytest.fixture(scope="module")
def cases():
    """{name: (case, its oracle)}: computed once, shared, never changed"""
    return {c["name"]: (c, S.oracle(c)) for c in S.build_cases()}


@pytest.fixture(scope="module")
def score_tables(cases):
    """{end_idx: ScoreRefs on the device} of the cases' one corpus"""
    from capmi.devscore import ScoreRefs
    corpus = cases["edges_end1"][0]["references"]
    return {end: ScoreRefs.build(corpus, end_idx=end, device=DEV) for end in (None, S.END)}


def _run(case, refs, rows=None):
    """capmi_caption_stats on the case's table (or on the rows ``rows`` of it, n = 1): host stats, bleu, rouge"""
    from capmi.devscore import DeviceCaptionScorer
    tab, lens = S.token_table(case)
    n, keys = case["n"], np.asarray(case["img_key"], dtype=np.int32)
    if rows is not None:
        tab, lens, keys, n = tab[:, rows], lens[rows], keys[[r // case["n"] for r in rows]], 1
    out = DeviceCaptionScorer(refs).score_table(_dev(tab), _dev(lens), _dev(keys), n=n, score_end=bool(case["score_end"]))
    torch.cuda.synchronize()
    return out["stats"].cpu().numpy(), out["bleu"].cpu().numpy(), out["rouge"].cpu().numpy(), out["cider"].cpu().numpy()


@pytest.mark.parametrize("name", ["edges_end1", "edges_end0", "n5", "t1_r1", "t1_empty", "no_end"])
def test_stats_and_scores_match_the_oracle(cases, score_tables, name):
    case, (want_stats, want_bleu, want_rouge) = cases[name]
    stats, bleu, rouge, cider = _run(case, score_tables[case["end_idx"]])
    assert stats.shape == want_stats.shape and stats.dtype == np.int32
    wrong = np.flatnonzero((stats != want_stats).any(axis=1))
    assert wrong.size == 0, (name, wrong[:5], stats[wrong[:5]], want_stats[wrong[:5]])
    ub, ur = S.ulps32(bleu, want_bleu), S.ulps32(rouge, want_rouge)
    print(f"{name}: R {case['R']} T {case['T']} n {case['n']}: bleu max {ub.max():.2f} ulp, rouge max {ur.max():.2f} "
          f"ulp; {int((want_rouge == 0).sum())} rows of ROUGE-L 0, {int(np.isnan(want_rouge).sum())} off the table")
    assert ub.max() <= 1.0 and ur.max() <= 1.0, (name, ub.max(), ur.max())
    assert (rouge[want_rouge == 0] == 0).all()
    off = np.isnan(want_rouge)
    assert np.isnan(bleu[off]).all() and np.isnan(rouge[off]).all() and np.isnan(cider[off]).all()
    assert np.isfinite(cider[~off]).all()


def test_a_row_scores_the_same_alone_and_run_to_run(cases, score_tables):
    for name in ("edges_end1", "n5"):
        case = cases[name][0]
        refs = score_tables[case["end_idx"]]
        first, again = _run(case, refs), _run(case, refs)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
        for r in range(0, case["R"], 7):
            alone = _run(case, refs, rows=[r])
            for a, b in zip(first[:3], alone[:3]):
                assert a[r].tobytes() == b[0].tobytes(), (name, r, a[r], b[0])


def _cider_bound(table, hyps, keys):
    """(the bound of tests/test_gpu_scst.py for these rows, their fp64 rewards): four times the float32
    restatement's largest error, at least one fp32 ulp at 10"""
    from capmi.scst import cider_rewards_host
    want = cider_rewards_host(table, hyps, keys, True, None)
    worst = max(abs(SC.reward_f32(table, h, k) - w) for h, k, w in zip(hyps, keys, want))
    return max(4 * worst, SC.ULP_AT_10), want


def _check_corpus_scores(got, want, references, hypotheses, what):
    """BLEU / ROUGE-L 1e-9 relative to ``want``; CIDEr under the reward kernel's bound on this corpus"""
    from capmi.devscore import ScoreRefs, _cider_listing
    assert set(got) == {"Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"}
    assert all(isinstance(v, float) for v in got.values())
    for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L"):
        print(f"{what} {k}: device {got[k]:.12g} want {want[k]:.12g}")
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (what, k, got[k], want[k])
    table = ScoreRefs.build([_cider_listing([tuple(r) for r in refs]) for refs in references]).cider
    b, rows = _cider_bound(table, hypotheses, range(len(hypotheses)))
    assert abs(math.fsum(rows) / len(rows) - want["CIDEr"]) <= 1e-9 * abs(want["CIDEr"])  # the table is the corpus's
    print(f"{what} CIDEr: device {got['CIDEr']:.9g} want {want['CIDEr']:.9g}, bound {b:.3e}")
    assert abs(got["CIDEr"] - want["CIDEr"]) <= b, (what, got["CIDEr"], want["CIDEr"], b)


@pytest.mark.parametrize("case", ["corpus", "single_image"])
def test_caption_scores_device_on_the_reference_scorers_fixture(case):
    from capmi.devscore import caption_scores_device
    with open(os.path.join(HERE, "golden", "caption_scores.json")) as f:
        c = json.load(f)[case]
    got = caption_scores_device(c["references"], c["hypotheses"], DEV)
    _check_corpus_scores(got, c["scores"], c["references"], c["hypotheses"], case)


def test_caption_scores_device_with_unequally_repeated_references():
    """one reference listed twice next to another listed once: CIDEr's mean weighs the listing, BLEU / ROUGE-L the
    distinct references"""
    from capmi.devscore import caption_scores_device
    from capmi.scoring import caption_scores
    refs = [[[5, 6, 7, 8], [5, 6, 7, 8], [5, 9, 7]], [[4, 5, 6]] * 3, [[9, 9, 8], [7]]]
    hyps = [[5, 6, 7], [4, 5, 5, 6], [9, 8]]
    _check_corpus_scores(caption_scores_device(refs, hyps, DEV), caption_scores(refs, hyps), refs, hyps, "repeats")


@pytest.mark.parametrize("R", [1, 65, 1000])
def test_reward_mix(R):
    from capmi import kernels as K
    rng = np.random.default_rng(R)
    cider = (rng.random(R) * 10).astype(np.float32)
    bleu = rng.random((R, 4)).astype(np.float32)
    rouge = rng.random(R).astype(np.float32)
    if R > 4:
        cider[1], bleu[2, 3], rouge[3], bleu[4, 0] = np.nan, np.nan, np.nan, np.nan  # column 0 is not read
    for w in (WEIGHTS, (0.0, 1.0, 0.0), (-2.0, 3.5, 1e-3)):
        out = torch.full((R,), -7.0, device=DEV)
        K.reward_mix(_dev(cider), _dev(bleu), _dev(rouge), R, *w, out)
        got = out.cpu().numpy()
        want = S.mix64(w, cider, bleu[:, 3], rouge)
        assert S.ulps32(got, want).max() <= 1.0, (R, w)
        assert np.array_equal(np.isnan(got), np.isnan(want))
    if R > 4:
        assert np.isnan(got[1:4]).all() and np.isfinite(got[4])


# --------------------------------------------------------------------------------------------------- the steps
def _baseline_e2e(graph=False, baseline="mean", **kw):
    """tests/test_gpu_scst.py's peaked toy decoder and its own samples as references, on ScoreRefs"""
    from capmi.devscore import ScoreRefs
    from capmi.sample import BaselineBatchedSampler
    from capmi.scst import BaselineSelfCriticalStep
    from test_gpu_scst import E2E
    M, H, V, B, n, ms = (E2E[k] for k in ("M", "H", "V", "B", "n", "ms"))
    start, end = V - 3, V - 2
    dec, _ = BC.decoder(M, H, V, 5, DEV, fc_scale=E2E["fc_scale"], end_bias=E2E["end_bias"], end_idx=end)
    dec.fine_tune_embeddings(False)  # its scatter-add is atomic: the bits would depend on the order
    feats = t(gen.uniform(5, "feats", (B, M), -1, 1)).to(DEV)
    refs = [[] for _ in range(B)]
    for seed in (101, 202):
        for b, per in enumerate(BaselineBatchedSampler(dec, 1).sample(feats, start, end, max_steps=ms, seed=seed)):
            refs[b].append([w for w in per[0]["seq"] if w not in (start, end, 0)])
    table = ScoreRefs.build(refs, end_idx=end, device=DEV)
    step = BaselineSelfCriticalStep(TS.Identity(), dec, TS._adam(dec), table if kw.get("reward_mix") else table.cider,
                                    num_samples=n, baseline=baseline, max_steps=ms, graph=graph, start_idx=start,
                                    end_idx=end, pad_idx=0, **kw)
    return step, dec, feats, table, (B, n, V)


def _attention_e2e(graph=False, baseline="mean", **kw):
    """tests/test_gpu_scst_attention.py's toy decoder, likewise"""
    from capmi.devscore import ScoreRefs
    from capmi.sample import BatchedSampler
    from capmi.scst import AttentionSelfCriticalStep
    _, _, P, A, D, M, V, E = TA.SMALL
    B, n, ms = TA.E2E["B"], TA.E2E["n"], TA.E2E["ms"]
    start, end = V - 3, V - 2
    dec, _ = TA._decoder(A, D, M, V, E, 5, fc_scale=TA.E2E["fc_scale"], end_bias=TA.E2E["end_bias"],
                         train_embedding=False)
    feats = TA._feats(B, P, E).to(DEV)
    refs = [[] for _ in range(B)]
    for seed in (101, 202):
        for b, per in enumerate(BatchedSampler(dec, 1).sample(feats, start, end, max_steps=ms, seed=seed)):
            refs[b].append([w for w in per[0]["seq"] if w not in (start, end, 0)])
    table = ScoreRefs.build(refs, end_idx=end, device=DEV)
    step = AttentionSelfCriticalStep(TA.Feats(), dec, TA._adam(dec), table if kw.get("reward_mix") else table.cider,
                                     num_samples=n, baseline=baseline, max_steps=ms, graph=graph, start_idx=start,
                                     end_idx=end, pad_idx=0, **kw)
    return step, dec, feats, table, (B, n, V)


MAKE = dict(baseline=_baseline_e2e, attention=_attention_e2e)


def _components64(table, tokens, lens, keys):
    """the fp64 oracle's (cider, bleu4, rouge_l) of the rows of a token table, END scored"""
    from capmi.scoring import bleu, rouge_l
    from capmi.scst import cider_rewards_host, hyps_from_table
    hyps = hyps_from_table(tokens.cpu(), lens.cpu())
    cider = np.array(cider_rewards_host(table.cider, hyps, keys, True, table.end_idx))
    refs = [table.cider.references[k] for k in keys]
    bleu4 = np.array([bleu([r], [h])[3] for r, h in zip(refs, hyps)])
    rouge = np.array([rouge_l([r], [h]) for r, h in zip(refs, hyps)])
    return cider, bleu4, rouge


def _mix_bound(bound_cider, want, bleu4, rouge):
    """what the mix may differ by: the reward kernel's bound, one fp32 ulp of bleu4 and of rouge, one of the sum"""
    wc, wb, wr = (abs(w) for w in WEIGHTS)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    return wc * bound_cider + wb * ulp(bleu4) + wr * ulp(rouge) + ulp(want)


@pytest.mark.parametrize("model", ["baseline", "attention"])
@pytest.mark.parametrize("baseline", ["mean", "greedy"])
def test_step_with_a_reward_mix_against_the_oracles_components(bound, model, baseline):  # noqa: F811
    step, dec, feats, table, (B, n, V) = MAKE[model](baseline=baseline, reward_mix=MIX)
    loss = step(feats, list(range(B)), seed=7, update=False)
    torch.cuda.synchronize()
    last, sc = step.last, step._sc[B]
    assert math.isfinite(float(loss))
    keys = [r // n for r in range(B * n)]
    cider, bleu4, rouge = _components64(table, last["tokens"], last["lens"], keys)
    print(f"{model} {baseline}: mean CIDEr-D {cider.mean():.3f} BLEU-4 {bleu4.mean():.3f} ROUGE-L {rouge.mean():.3f}")
    assert (cider > 0).mean() >= 0.5 and (rouge > 0).mean() >= 0.5 and np.ptp(bleu4) > 0  # the mix tests something
    assert np.abs(last["cider"].cpu().numpy() - cider).max() <= bound
    assert S.ulps32(last["bleu4"].cpu().numpy(), bleu4).max() <= 1.0
    assert S.ulps32(last["rouge_l"].cpu().numpy(), rouge).max() <= 1.0
    want = S.mix64(WEIGHTS, cider, bleu4, rouge)
    err = np.abs(last["rewards"].cpu().numpy().astype(np.float64) - want)
    tol = _mix_bound(bound, want, bleu4, rouge)
    print(f"{model} {baseline}: mixed reward max abs error {err.max():.3e} (least bound {tol.min():.3e})")
    assert (err <= tol).all()
    assert abs(float(last["reward_mean"]) - want.mean()) <= tol.max()
    if baseline == "greedy":
        g = _components64(table, sc.gtokens, sc.glens, list(range(B)))
        wantg = S.mix64(WEIGHTS, *g)
        errg = np.abs(last["greedy_rewards"].cpu().numpy().astype(np.float64) - wantg)
        assert (errg <= _mix_bound(bound, wantg, g[1], g[2])).all()
        adv = (want.reshape(B, n) - wantg[:, None]).reshape(-1)
        assert np.abs(last["adv"].cpu().numpy() - adv).max() <= 2 * tol.max()
    before = {k: q.detach().clone() for k, q in dec.named_parameters() if q.requires_grad}
    step(feats, list(range(B)), seed=8)
    torch.cuda.synchronize()
    assert step.opt.step_count == 1
    for k, q in dec.named_parameters():
        if q.requires_grad:
            assert bool(torch.isfinite(q).all()) and not torch.equal(q, before[k]), k


def _three(model, graph, **kw):
    step, dec, feats, _, (B, _, _) = MAKE[model](graph, **kw)
    losses = [step(feats, list(range(B)), seed=30 + s).clone() for s in range(3)]
    torch.cuda.synchronize()
    return step, torch.cat(losses).cpu(), [q.detach().cpu() for q in dec.parameters()]


@pytest.mark.parametrize("model", ["baseline", "attention"])
def test_mixed_step_graph_replay_equals_eager_bit_for_bit(model):
    s_e, l_e, p_e = _three(model, False, reward_mix=MIX)
    s_g, l_g, p_g = _three(model, True, reward_mix=MIX)
    assert s_e.counts == {"replay": 0, "eager": 3, "capture": 0}
    assert s_g.counts == {"replay": 2, "eager": 0, "capture": 1}, s_g.counts
    assert bool(torch.isfinite(l_e).all()) and len(set(l_e.tolist())) == 3
    assert torch.equal(l_e, l_g), (l_e, l_g)
    for a, b in zip(p_e, p_g):
        assert torch.equal(a, b)
    assert torch.equal(s_e.last["rewards"].cpu(), s_g.last["rewards"].cpu())


@pytest.mark.parametrize("model", ["baseline", "attention"])
def test_reward_mix_none_is_the_step_without_the_keyword(model):
    s_0, l_0, p_0 = _three(model, False)
    s_n, l_n, p_n = _three(model, False, reward_mix=None)
    assert "bleu4" not in s_n.last and set(s_n.last) == set(s_0.last)
    assert torch.equal(l_0, l_n)
    for a, b in zip(p_0, p_n):
        assert torch.equal(a, b)
    # and a mix of CIDEr-D alone rounds the same reward once more through fp64: the same rewards
    s_c, _, _ = _three(model, False, reward_mix=dict(cider=1.0))
    assert torch.equal(s_c.last["rewards"].cpu(), s_0.last["rewards"].cpu())


def test_a_reward_mix_needs_score_refs():
    from capmi.scst import BaselineSelfCriticalStep
    dec, _ = BC.decoder(16, 24, 40, 5, DEV)
    with pytest.raises(ValueError, match="ScoreRefs"):
        BaselineSelfCriticalStep(TS.Identity(), dec, TS._adam(dec), TA._dummy_refs(40), reward_mix=MIX)


# --------------------------------------------------------------------------------------------------- validation
def _compare_scorers(run, what):
    host, dev = run("host"), run("device")
    assert host["losses"] == dev["losses"] and host["loss"] == dev["loss"]
    assert host["references"] == dev["references"] and host["hypotheses"] == dev["hypotheses"]
    assert host["top1_acc"] == dev["top1_acc"] and host["top5_acc"] == dev["top5_acc"]
    _check_corpus_scores({k: dev[k] for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")}, host,
                         host["references"], host["hypotheses"], what)


def test_attention_evaluate_batched_with_the_device_scorer():
    from models.attention import evaluate_batched
    c = EC.E2E
    dec, _ = make_decoder(c["A"], c["D"], c["M"], c["V"], 79, DEV)
    items = EC.e2e_inputs(79)
    enc = lambda x: x  # noqa: E731  (features stand in for images: identity encoder)
    enc.eval = lambda: None

    def run(scorer):
        args = types.SimpleNamespace(print_freq=3, checkpoint=None, max_caption_length=-1, scorer=scorer)
        return evaluate_batched(DEV, args, enc, dec, dataset=items, batch_size=c["batch_size"])
    _compare_scorers(run, "attention")


def test_baseline_evaluate_batched_with_the_device_scorer():
    from models.baseline import evaluate_batched
    c = BC.E2E
    dec, _ = BC.decoder(c["M"], c["H"], c["V"], 75, DEV)
    dataset = BC.ListDataset(BC.e2e_inputs(75), c["V"])

    def run(scorer):
        args = types.SimpleNamespace(dataset=dataset, print_freq=3, checkpoint=None, scorer=scorer)
        return evaluate_batched(DEV, args, BC.IdentityEncoder(), dec, dataset=dataset, batch_size=c["batch_size"])
    _compare_scorers(run, "baseline")


# --------------------------------------------------------------------------------------------------- train
def test_train_self_critical_with_a_reward_mix(monkeypatch, tmp_path, capsys):
    """tests/test_gpu_scst.py's tiny run with ``args.sc_reward_mix`` set: ScoreRefs tables, the mixed step in its
    graph, the three component means in the log line"""
    import models.baseline as MB
    from capmi.devscore import ScoreRefs
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
                                 model_name="scmix", model="baseline", checkpoint="ce_0.pth.tar", self_critical=True,
                                 sc_samples=3, sc_baseline="greedy", sc_temperature=1.0, sc_top_k=0, sc_max_len=8,
                                 sc_reward_mix=MIX)
    MB.train_self_critical(torch.device("cuda"), args)
    out = capsys.readouterr().out
    assert all(k in out for k in ("Reward", "Greedy", "CIDEr-D", "BLEU-4", "ROUGE-L")), out
    step = MB.train_self_critical.last_step
    assert isinstance(step.refs, ScoreRefs) and step.reward_mix == WEIGHTS
    assert step.counts == {"replay": 1, "eager": 0, "capture": 1}, step.counts  # two batches of four images
    ck = torch.load(os.path.join("checkpoints", "scmix_0.pth.tar"), weights_only=True)
    assert all(math.isfinite(x) for x in ck["metrics"]["epoch_losses"][0] + ck["metrics"]["epoch_rewards"][0])
    last = step.last
    want = S.mix64(WEIGHTS, last["cider"].cpu().numpy(), last["bleu4"].cpu().numpy(), last["rouge_l"].cpu().numpy())
    assert S.ulps32(last["rewards"].cpu().numpy(), want).max() <= 1.0
