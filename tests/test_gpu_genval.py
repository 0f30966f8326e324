"""GPU: validation on generated captions -- capmi_beam_backtrack (csrc/beam.hip) against a Python walk over a
simulated beam state, ``search_device`` against ``search`` on both captioners, ``evaluate_generated`` against the host
path composed per batch, and eval.py --decode beam end to end."""
import functools
import itertools
import json
import math
import random
import types

import numpy as np
import pytest
import torch

import baseline_cases as BLC
import beam_cases as BC
import gen
from helpers import t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, START, END, PAD = 50, 47, 48, 0  # synthetic_vocab(50)
GARBAGE = -12345                     # what a never-written entry of the state holds here
EINVAL, ERANGE = 1001, 1003


# ---------------------------------------------------------------------------------------------
# 1. capmi_beam_backtrack against a Python walk
# ---------------------------------------------------------------------------------------------
def simulate(B, k, T, steps, ends, word_of, score_of, seed):
    """The state capmi_beam_advance leaves after ``steps`` steps, built on the host: per step and image every
    selection slot r < live takes a seeded parent among the rows live before it and the word ``word_of(i, t, r)``
    (END where ``ends(i, t, r)``), with the score ``score_of(i, t, r)``. Entries no step writes hold GARBAGE."""
    rng = random.Random(seed)
    R = B * k
    st = dict(bp=np.full((T, 3, R), GARBAGE, np.int32), fin_count=np.zeros(B, np.int32),
              fin_step=np.full((B, k), GARBAGE, np.int32), fin_slot=np.full((B, k), GARBAGE, np.int32),
              fin_score=np.full((B, k), np.nan, np.float32), live=np.full(B, k, np.int32),
              scores=np.zeros((B, k), np.float32), steps=steps, B=B, k=k, T=T)
    for t_ in range(steps):
        for i in range(B):
            s = int(st["live"][i])
            n = 0
            for r in range(s):
                par = 0 if t_ == 0 else rng.randrange(s)
                w = END if ends(i, t_, r) else word_of(i, t_, r)
                v = np.float32(score_of(i, t_, r))
                st["bp"][t_, 0, i * k + r], st["bp"][t_, 1, i * k + r] = par, w
                if w == END:
                    nf = int(st["fin_count"][i])
                    if nf < k:
                        st["fin_step"][i, nf], st["fin_slot"][i, nf], st["fin_score"][i, nf] = t_, r, v
                        st["fin_count"][i] = nf + 1
                else:
                    st["bp"][t_, 2, i * k + n] = r
                    st["scores"][i, n] = v
                    n += 1
            st["live"][i] = n
    return st


def walk(st, i, t_, slot):
    """``_BeamState.finish``'s walk: (words, alpha rows) of the beam selected at step t_ as ``slot``."""
    k, R = st["k"], st["B"] * st["k"]
    words, rows = [], []
    while True:
        row = int(st["bp"][t_, 0, i * k + slot])
        words.append(int(st["bp"][t_, 1, i * k + slot]))
        rows.append(t_ * R + i * k + row)
        if t_ == 0:
            break
        t_ -= 1
        slot = int(st["bp"][t_, 2, i * k + row])
    return words[::-1], rows[::-1]


def keys64(st, i, alpha):
    nf = int(st["fin_count"][i])
    return [float(st["fin_score"][i, q]) / float(int(st["fin_step"][i, q]) + 1) ** alpha for q in range(nf)]


def expected(st, emit_end, drop, fallback_live, alpha, broken=()):
    """tokens (T, B), lens, finished, score, alpha_rows (T, B) by the Python walk; images in ``broken`` hold an
    index outside its range and come out empty."""
    B, k, T = st["B"], st["k"], st["T"]
    tokens, rows_out = np.full((T, B), -1, np.int32), np.full((T, B), -1, np.int32)
    lens, fin, score = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    for i in range(B):
        if i in broken:
            continue
        nf = int(st["fin_count"][i])
        if nf:
            key = [float(x) for x in st["fin_score"][i, :nf]] if alpha == 0 else keys64(st, i, alpha)
            q = key.index(max(key))
            words, rows = walk(st, i, int(st["fin_step"][i, q]), int(st["fin_slot"][i, q]))
            assert words[-1] == END
            if not emit_end:
                words = words[:-1]
            fin[i], score[i] = 1, st["fin_score"][i, q]
        elif fallback_live and st["live"][i] > 0 and st["steps"] > 0:
            words, rows = walk(st, i, st["steps"] - 1, int(st["bp"][st["steps"] - 1, 2, i * k]))
            score[i] = st["scores"][i, 0]
        else:
            continue
        words = [w for w in words if w not in drop]
        tokens[:len(words), i], lens[i] = words, len(words)
        rows_out[:len(rows), i] = rows
    return tokens, lens, fin, score, rows_out


def run_kernel(st, emit_end, drop, fallback_live, alpha, with_rows):
    from capmi import kernels as K
    B, k, T = st["B"], st["k"], st["T"]
    d = {n: torch.from_numpy(st[n]).to(DEV) for n in ("bp", "fin_count", "fin_step", "fin_slot", "fin_score", "live",
                                                      "scores")}
    i32 = dict(dtype=torch.int32, device=DEV)
    tokens, rows = torch.full((T, B), 77, **i32), torch.full((T, B), 77, **i32) if with_rows else None
    lens, fin = torch.full((B,), 77, **i32), torch.full((B,), 77, **i32)
    score = torch.full((B,), 77.0, device=DEV)
    drop = tuple(drop) + (-1,) * (2 - len(drop))
    K.beam_backtrack(d["bp"], d["fin_count"], d["fin_step"], d["fin_slot"], d["fin_score"], d["live"], d["scores"],
                     st["steps"], B, k, T, END, tokens, lens, fin, score, alpha_rows=rows, drop_a=drop[0],
                     drop_b=drop[1], emit_end=emit_end, fallback_live=fallback_live, length_alpha=alpha)
    torch.cuda.synchronize()
    return (tokens.cpu().numpy(), lens.cpu().numpy(), fin.cpu().numpy(), score.cpu().numpy(),
            None if rows is None else rows.cpu().numpy())


def check_all_modes(st, drop, broken=()):
    for emit_end, fallback, alpha, with_rows in itertools.product((0, 1), (0, 1), (0.0, 0.7), (False, True)):
        want = expected(st, emit_end, drop, fallback, alpha, broken)
        got = run_kernel(st, emit_end, drop, fallback, alpha, with_rows)
        what = f"emit_end {emit_end} fallback {fallback} alpha {alpha} rows {with_rows}"
        for name, g, w in zip(("tokens", "lens", "finished"), got, want):
            assert np.array_equal(g, w), (what, name, g, w)
        assert got[3].tobytes() == want[3].tobytes(), (what, "score", got[3], want[3])
        if with_rows:
            assert np.array_equal(got[4], want[4]), (what, "alpha_rows")


def assert_keys_are_separated(st, alpha):
    """The construction the fp64 key comparison rests on: two finished beams of an image have keys more than 1e-6
    apart (relative), or the same score at the same step (then the keys are the same arithmetic)."""
    for i in range(st["B"]):
        key = keys64(st, i, alpha)
        for a, b in itertools.combinations(range(len(key)), 2):
            same = (st["fin_score"][i, a].tobytes() == st["fin_score"][i, b].tobytes()
                    and st["fin_step"][i, a] == st["fin_step"][i, b])
            assert same or abs(key[a] - key[b]) > 1e-6 * max(abs(key[a]), abs(key[b])), (i, a, b, key)


def small_state():
    """B = 5, k = 3, T = 7, 6 steps run. Image 0: never ends. 1: slot 1 ends at step 0 with the best score. 2: slots 0
    and 1 end at step 2 with bit-equal scores, the last beam at step 4 with a lower one. 3: the words of steps 0 and 1
    are START and PAD; one beam ends at step 4. 4: all three beams end (steps 1, 3, 3)."""
    plan = {1: {(0, 1), (3, 0)}, 2: {(2, 0), (2, 1), (4, 0)}, 3: {(4, 0)}, 4: {(1, 2), (3, 0), (3, 1)}}
    rng = random.Random(5)
    noise = {(i, t_, r): rng.random() for i in range(5) for t_ in range(7) for r in range(3)}

    def score_of(i, t_, r):
        if i == 2 and t_ == 2:
            return -1.25  # the tie
        if i == 1 and t_ == 0:
            return -0.5
        return -(t_ + 1) - 0.1 * r - 0.05 * noise[i, t_, r]  # descending in the slot, as a selection is

    def word_of(i, t_, r):
        if i == 3 and t_ < 2:
            return (START, PAD)[t_]
        return 3 + int(noise[i, t_, r] * 40)

    return simulate(5, 3, 7, 6, lambda i, t_, r: (t_, r) in plan.get(i, ()), word_of, score_of, seed=11)


def test_backtrack_matches_the_python_walk_on_the_five_images():
    st = small_state()
    assert st["fin_count"].tolist() == [0, 2, 3, 1, 3] and st["live"].tolist() == [3, 1, 0, 2, 0]
    assert st["fin_step"][1, 0] == 0 and st["fin_score"][1, 0] == max(st["fin_score"][1, :2])
    assert st["fin_score"][2, 0].tobytes() == st["fin_score"][2, 1].tobytes()
    assert st["fin_score"][2, 1] > st["fin_score"][2, 2] and st["fin_slot"][2, :2].tolist() == [0, 1]
    words3, _ = walk(st, 3, int(st["fin_step"][3, 0]), int(st["fin_slot"][3, 0]))
    assert words3[:2] == [START, PAD] and words3[-1] == END
    assert_keys_are_separated(st, 0.7)
    check_all_modes(st, (START, PAD))
    check_all_modes(st, ())
    # what the cases are there for, read off the expectation itself
    tokens, lens, fin, score, rows = expected(st, 0, (START, PAD), 0, 0.0)
    assert lens.tolist()[0] == 0 and fin.tolist() == [0, 1, 1, 1, 1] and lens[1] == 0 and lens[3] == 2
    assert (rows[:5, 3] >= 0).all() and rows[5, 3] == -1  # five steps on image 3's path, two words kept
    assert (tokens[:, 2] == expected(st, 0, (), 0, 0.0)[0][:, 2]).all() and score[2] == np.float32(-1.25)
    assert walk(st, 2, 2, 0)[0][:-1] == tokens[:lens[2], 2].tolist()  # the first of the tie
    live = expected(st, 1, (START, PAD), 1, 0.0)
    assert live[1][0] == 6 and live[2][0] == 0 and live[3][0] == st["scores"][0, 0]


def test_backtrack_on_a_second_workgroup_at_beam_kmax():
    B, k, T = 65, 16, 7
    rng = random.Random(3)
    noise = {(i, t_, r): rng.random() for i in range(B) for t_ in range(T) for r in range(k)}
    # distinct scores everywhere: a multiple of 2^-10 per (step, slot) plus the image's own offset
    st = simulate(B, k, T, T, lambda i, t_, r: i % 7 != 0 and noise[i, t_, r] < 0.12 + 0.3 * (i % 3 == 0),
                  lambda i, t_, r: [START, PAD, 5, 9, 30][int(noise[i, t_, r] * 1000) % 5],
                  lambda i, t_, r: -(t_ * 1.5 + 1) - (r + 1) / 64.0 - (i % 5) / 1024.0, seed=4)
    assert st["fin_count"].max() == k and (st["fin_count"] == 0).sum() >= 10 and st["fin_count"][64] > 0
    assert ((st["fin_count"] == 0) & (st["live"] > 0)).any()
    assert_keys_are_separated(st, 0.7)
    assert_keys_are_separated(st, 0.0)
    check_all_modes(st, (START, PAD))


def test_backtrack_gives_an_empty_caption_for_an_index_outside_its_range():
    """The state is read defensively: a finished slot of k + 3 (image 1), a parent row of k (image 3) and a finished
    step of ``steps`` (image 4) are rejected before anything is read through them; the neighbours are unaffected."""
    st = small_state()
    k = st["k"]
    st["fin_slot"][1, 0] = k + 3
    assert st["fin_count"][3] == 1 and st["fin_step"][3, 0] == 4  # image 3's path passes step 2; all k rows live there
    st["bp"][2, 0, 3 * k:4 * k] = k  # every slot of that step: whichever the path takes
    st["fin_step"][4, :] = st["steps"]
    check_all_modes(st, (START, PAD), broken=(1, 3, 4))


def test_backtrack_argument_checks():
    from capmi import kernels as K
    from capmi._lib import CapmiError, lib
    st = small_state()
    d = {n: torch.from_numpy(st[n]).to(DEV) for n in ("bp", "fin_count", "fin_step", "fin_slot", "fin_score", "live",
                                                      "scores")}
    i32 = dict(dtype=torch.int32, device=DEV)
    tokens, lens, fin = torch.full((7, 5), 77, **i32), torch.full((5,), 77, **i32), torch.full((5,), 77, **i32)
    score = torch.full((5,), 77.0, device=DEV)
    p = lambda x: x.data_ptr()  # noqa: E731

    def call(steps=6, B=5, k=3, T=7, end=END, alpha=0.0, bp=p(d["bp"]), tok=p(tokens), fs=p(d["fin_score"])):
        return lib.capmi_beam_backtrack(bp, p(d["fin_count"]), p(d["fin_step"]), p(d["fin_slot"]), fs, p(d["live"]),
                                        p(d["scores"]), steps, B, k, T, end, -1, -1, 0, 0, alpha, tok, p(lens), p(fin),
                                        p(score), None, None)

    assert call(bp=None) == EINVAL and call(tok=None) == EINVAL and call(fs=None) == EINVAL
    assert call(B=0) == EINVAL and call(k=0) == EINVAL and call(k=17) == EINVAL and call(T=0) == EINVAL
    assert call(steps=-1) == EINVAL and call(steps=8) == EINVAL and call(end=-1) == EINVAL
    assert call(alpha=-1e-9) == EINVAL and call(alpha=float("nan")) == EINVAL
    assert call(B=1 << 24, k=16, T=3, steps=3) == ERANGE
    with pytest.raises(CapmiError):
        K.beam_backtrack(d["bp"], d["fin_count"], d["fin_step"], d["fin_slot"], d["fin_score"], d["live"], d["scores"],
                         8, 5, 3, 7, END, tokens, lens, fin, score)
    torch.cuda.synchronize()
    assert int(tokens.min()) == 77 and int(lens.min()) == 77  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert lens.cpu().tolist() == expected(st, 0, (), 0, 0.0)[1].tolist()


# ---------------------------------------------------------------------------------------------
# 2. search_device against search, both captioners
# ---------------------------------------------------------------------------------------------
K_BEAMS, MAX_STEPS = 3, 6
STRIP = {START, END, PAD}


def _strip(seq):
    return [w for w in seq if w not in STRIP]


def _attention_case():
    """Chosen on the CPU (tests/beam_cases.py::beam_loop, k = 3, max_steps = 6): decoder seed 62, fc x 8, END bias
    0.3; images 1 and 4 finish beams, 0, 2 and 3 do not; every selection margin is above 4e-3."""
    dec, _ = BC.tuned_decoder(32, 32, 16, V, 62, 8.0, 0.3, END, DEV)
    return dec, BC.features([62 + 100 * b for b in range(5)]).to(DEV)


def _baseline_case():
    """Chosen on the CPU (tests/baseline_cases.py::beam_loop): seed 48, linear x 60, END bias 2; image 1 finishes no
    beam within 6 steps, the others do; margins above 4e-3."""
    dec, _ = BLC.decoder(16, 24, V, 48, DEV, fc_scale=60.0, end_bias=2.0, end_idx=END)
    return dec, torch.stack([t(gen.uniform(48 + i, "feats", (16,), -1, 1)) for i in range(5)]).to(DEV)


@pytest.mark.parametrize("model", ["attention", "baseline"])
def test_search_device_matches_search(model):
    from capmi.beam import BaselineBatchedBeamSearch, BatchedBeamSearch
    dec, feats = _attention_case() if model == "attention" else _baseline_case()
    bs = (BatchedBeamSearch if model == "attention" else BaselineBatchedBeamSearch)(dec, K_BEAMS)
    kw = dict(return_alphas=False) if model == "attention" else {}
    host = bs.search(feats, START, END, max_steps=MAX_STEPS, return_all=True, sync_every=2, **kw)
    live, host_stats = bs.last_live, dict(bs.last_stats)
    ok = [r[2] for r in host]
    print(f"{model}: finished {ok}, steps {host_stats}")
    assert any(ok) and not all(ok)  # the case: an image that does not finish within max_steps beside ones that do
    for fallback in (False, True):
        out = bs.search_device(feats, START, END, max_steps=MAX_STEPS, sync_every=2, drop=(START, PAD),
                               fallback_live=fallback)
        assert bs.last_stats == {"steps": host_stats["steps"], "host_syncs": host_stats["host_syncs"] - 1}
        assert bs.last_stats["host_syncs"] == (host_stats["steps"] - (host_stats["steps"] == MAX_STEPS + 1)) // 2
        assert out["tokens"].shape == (MAX_STEPS + 1, 5) and out["tokens"].dtype == torch.int32
        assert all(out[n].is_cuda for n in ("tokens", "lens", "finished", "score", "steps"))
        assert int(out["steps"]) == host_stats["steps"]
        tokens, lens = out["tokens"].cpu(), out["lens"].cpu().tolist()
        assert out["finished"].cpu().tolist() == [int(x) for x in ok]
        for i, (seq, _, done, (done_seqs, done_scores)) in enumerate(host):
            got = tokens[:lens[i], i].tolist()
            assert (tokens[lens[i]:, i] == -1).all()
            if done:
                assert got == _strip(seq)
                want = np.float32(done_scores[done_seqs.index(seq)])
                assert np.float32(out["score"][i].item()).tobytes() == want.tobytes()
            elif fallback:
                assert got == _strip(live[i][0][0]) and len(live[i][0][0]) == MAX_STEPS + 2  # START + a word per step
                assert np.float32(out["score"][i].item()).tobytes() == np.float32(live[i][1][0]).tobytes()
            else:
                assert got == [] and float(out["score"][i]) == 0.0
    # END kept, nothing dropped: the host's sequence without its START
    out = bs.search_device(feats, START, END, max_steps=MAX_STEPS, emit_end=True)
    for i, (seq, _, done, _) in enumerate(host):
        n = int(out["lens"][i])
        assert out["tokens"][:n, i].tolist() == (seq[1:] if done else [])
    # the longest-normalised choice against the host's finished lists
    out = bs.search_device(feats, START, END, max_steps=MAX_STEPS, length_alpha=0.7, emit_end=True)
    for i, (_, _, done, (done_seqs, done_scores)) in enumerate(host):
        if done:
            key = [s / float(len(q) - 1) ** 0.7 for q, s in zip(done_seqs, done_scores)]  # len - 1 = step + 1
            order = sorted(key, reverse=True)
            assert len(order) < 2 or order[0] - order[1] > 1e-6 * abs(order[0])
            assert out["tokens"][:int(out["lens"][i]), i].tolist() == done_seqs[key.index(max(key))][1:]
    with pytest.raises(ValueError):
        bs.search_device(feats, START, END, drop=(1, 2, 3))
    with pytest.raises(ValueError):
        bs.search_device(feats, START, END, length_alpha=-1.0)


def test_search_device_rejects_bert_features():
    from capmi.beam import BatchedBeamSearch
    dec, feats = _attention_case()
    dec.use_bert = True
    with pytest.raises(NotImplementedError):
        BatchedBeamSearch(dec, K_BEAMS).search_device(feats, START, END)


# ---------------------------------------------------------------------------------------------
# 3. evaluate_generated against the host path, batch by batch
# ---------------------------------------------------------------------------------------------
class PixelFeatures:
    """A stand-in encoder: features are a fixed function of a few pixels, so the pass runs through the real loader,
    the ragged last batch and the device tables without a ResNet forward. (eval.py below runs the real encoders.)"""

    def __init__(self, model):
        self.model = model
        g = torch.Generator().manual_seed(17)
        self.W = (torch.rand(3, 2048, generator=g) - 0.35).to(DEV)

    def eval(self):
        return self

    def __call__(self, imgs):
        if self.model == "baseline":
            return (0.4 * imgs[:, 0, 0, :16]).contiguous()
        x = imgs[:, :, 8::16, 8::16].permute(0, 2, 3, 1)  # (B, 14, 14, 3)
        return torch.relu(x @ self.W).contiguous()


def _decoder(model):
    if model == "attention":
        return BC.tuned_decoder(32, 32, 16, V, 62, 8.0, 0.3, END, DEV)[0]
    # on the CPU loop 9 of the 13 images finish a beam within 6 steps under PixelFeatures; attention: 2 of 13
    return BLC.decoder(16, 24, V, 48, DEV, fc_scale=50.0, end_bias=1.5, end_idx=END)[0]


@functools.lru_cache(maxsize=None)
def _generated(model):
    import importlib
    from capmi.data import SyntheticCOCO
    mod = importlib.import_module(f"models.{model}")
    ds = SyntheticCOCO(13, V=V, L=8, ragged=True)
    args = types.SimpleNamespace(beam_size=K_BEAMS, max_decode_len=MAX_STEPS, length_alpha=0.0, print_freq=2,
                                 checkpoint=None)
    dec, enc = _decoder(model), PixelFeatures(model)
    got = mod.evaluate_generated(torch.device(DEV), args, enc, dec, dataset=ds, batch_size=4)
    args.max_decode_len = 64  # one word more than the scorer's hypothesis holds
    with pytest.raises(ValueError):
        mod.evaluate_generated(torch.device(DEV), args, enc, dec, dataset=ds, batch_size=4)
    return ds, dec, enc, got


@pytest.mark.parametrize("model", ["attention", "baseline"])
def test_evaluate_generated_matches_the_host_path(model):
    from capmi.beam import BaselineBatchedBeamSearch, BatchedBeamSearch
    from capmi.genval import PerImageView, build_refs
    from capmi.scoring import caption_scores
    from test_gpu_score import _check_corpus_scores
    ds, dec, enc, got = _generated(model)
    assert set(got) == {"Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "hypotheses", "image_keys",
                        "unfinished", "mean_length", "host_syncs", "captions_per_s"}
    assert json.loads(json.dumps(got)) == got and got["image_keys"] == list(range(13))
    # the host path: search() per batch of 4 (the last one holds image 12 alone), its walk and its lists
    bs = (BatchedBeamSearch if model == "attention" else BaselineBatchedBeamSearch)(dec, K_BEAMS)
    kw = dict(return_alphas=False) if model == "attention" else {}
    hyps, failures, syncs = [], 0, 0
    for b0 in range(0, 13, 4):
        imgs = torch.stack([ds[i][0] for i in range(b0, min(b0 + 4, 13))]).to(DEV)
        res = bs.search(enc(imgs), START, END, max_steps=MAX_STEPS, **kw)
        syncs += bs.last_stats["host_syncs"] - 1
        for i, (seq, _, done) in enumerate(res):
            failures += not done
            hyps.append(_strip(seq if done else bs.last_live[i][0][0]))
    print(f"{model}: {failures} of 13 unfinished, lengths {[len(h) for h in hyps]}")
    assert got["hypotheses"] == hyps
    if model == "baseline":  # both ways out of the back-trace are in the corpus (far from either end on the CPU)
        assert 0 < failures < 13
    assert got["unfinished"] == failures and got["host_syncs"] == syncs
    assert got["mean_length"] == sum(len(h) for h in hyps) / 13 and got["captions_per_s"] > 0
    _, references = build_refs(PerImageView(ds), STRIP, "cpu")
    assert [r[0] for r in references] == [_strip(ds[i][1].tolist()) for i in range(13)] and len(references[0]) == 5
    want = caption_scores(references, hyps)
    _check_corpus_scores({k: got[k] for k in want}, want, references, hyps, f"generated {model}")


# ---------------------------------------------------------------------------------------------
# 4. eval.py --decode beam
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["attention", "baseline"])
def test_eval_cli_decode_beam(model, tmp_path, monkeypatch):
    """eval.main --decode beam through the real encoder on 13 synthetic images, batch 4, from a checkpoint written
    by save_checkpoint: the JSON it writes is what it returns."""
    import eval as E
    from checkpoint import save_checkpoint
    from helpers import make_decoder
    from models.encoder import Encoder, EncoderAttention
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    if model == "attention":
        dec, enc = make_decoder(32, 32, 16, V, 9, "cpu")[0], EncoderAttention()
    else:
        dec, enc = BLC.decoder(16, 24, V, 9, "cpu")[0], Encoder(16)
    opt = types.SimpleNamespace(state_dict=lambda: {})
    save_checkpoint(types.SimpleNamespace(model_name="gen"), 0, enc, dec, None, opt, {}, verbose=False)
    out = E.main(["gen_0.pth.tar", "--model_type", model, "--decode", "beam", "--synthetic_size", "13", "--batch_size",
                  "4", "--vocab_size", str(V), "--synthetic_len", "8", "--max_decode_len", "6", "--print_freq", "10"])
    assert set(out) == {"Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "hypotheses", "image_keys",
                        "unfinished", "mean_length", "host_syncs", "captions_per_s"}
    assert len(out["hypotheses"]) == 13 and out["image_keys"] == list(range(13)) and 0 <= out["unfinished"] <= 13
    assert all(len(h) <= 7 and all(0 < w < V and w not in STRIP for w in h) for h in out["hypotheses"])
    assert all(math.isfinite(out[k]) and out[k] >= 0 for k in ("Bleu_1", "Bleu_4", "ROUGE_L", "CIDEr"))
    with open(tmp_path / "eval_data" / "gen_0.json") as f:
        assert json.load(f) == out
