"""GPU: capmi.beam.BaselineBatchedBeamSearch against the CPU beam loop of tests/baseline_cases.py.

Cases chosen on the CPU: the tiny decoder (M = 16, H = 24, V = 50) with linear.weight scaled and the END bias
raised so that beams finish. Seed 48, scale 60, k = 3: the fp64 and fp32 loops select identical beams, the
selection margin is 4.7e-3, the three images stop after 9 / 10 / 9 steps with every beam finished. Seed 2, scale
30: margin 3.3e-3 and image 0 still has a live beam at the step cap. The bar for comparing selections exactly is
the project's (tests/test_gpu_beam_batched.py): an oracle margin of at least 1e-3."""
import types

import pytest
import torch

import baseline_cases as BC
import gen
from helpers import t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, H, V = 16, 24, 50
START, END = 47, 48
MAX_STEPS = 20


def _close(got, want):
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


def _case(seed, scale, n_img, k):
    dec, p = BC.decoder(M, H, V, seed, DEV, fc_scale=scale, end_bias=2.0, end_idx=END)
    feats = torch.stack([t(gen.uniform(seed + i, "feats", (M,), -1, 1)) for i in range(n_img)])
    want = [BC.beam_loop(p, feats[i], k, START, END, MAX_STEPS, dtype=torch.float32) for i in range(n_img)]
    want64 = [BC.beam_loop(p, feats[i], k, START, END, MAX_STEPS, dtype=torch.float64) for i in range(n_img)]
    for a, b in zip(want, want64):  # preconditions: the selection is far from changing
        assert b["margin"] >= 1e-3, b["margin"]
        assert a["done_seqs"] == b["done_seqs"] and a["live_seqs"] == b["live_seqs"]
    return dec, feats, want64


def _check(got, live, want):
    seq, alphas, ok, (done_seqs, done_scores) = got
    assert alphas == [] and ok == want["ok"] and seq == want["seq"]
    assert done_seqs == want["done_seqs"]
    assert len(done_scores) == len(want["done_scores"])
    for g, w in zip(done_scores, want["done_scores"]):
        assert _close(g, w), (g, w)
    assert live[0] == want["live_seqs"]
    for g, w in zip(live[1], want["live_scores"]):
        assert _close(g, w), (g, w)


def test_batch_of_3_matches_the_cpu_loop_and_each_image_alone():
    from capmi.beam import BaselineBatchedBeamSearch
    dec, feats, want = _case(48, 60.0, 3, 3)
    assert [w["steps"] for w in want] == [9, 10, 9] and all(w["live_seqs"] == [] for w in want)
    assert [len(w["seq"]) for w in want] == [7, 9, 8]
    bs = BaselineBatchedBeamSearch(dec, 3)
    got = bs.search(feats.to(DEV), START, END, max_steps=MAX_STEPS, return_all=True, sync_every=8)
    # the host looks at the live count after steps 8 and 16; at 16 every image is done (10 steps needed)
    assert bs.last_stats == {"steps": 16, "host_syncs": 3}
    for i in range(3):
        _check(got[i], bs.last_live[i], want[i])
    plain = bs.search(feats.to(DEV), START, END, max_steps=MAX_STEPS, sync_every=2)
    assert bs.last_stats == {"steps": 10, "host_syncs": 6}
    assert [len(r) for r in plain] == [3, 3, 3] and [r[0] for r in plain] == [w["seq"] for w in want]
    for i in range(3):
        alone = bs.search(feats[i:i + 1].to(DEV), START, END, max_steps=MAX_STEPS, return_all=True)
        assert alone[0][0] == got[i][0] and alone[0][3][0] == got[i][3][0]
        assert all(_close(a, b) for a, b in zip(alone[0][3][1], got[i][3][1]))


def test_live_beams_at_the_step_cap():
    from capmi.beam import BaselineBatchedBeamSearch
    dec, feats, want = _case(2, 30.0, 3, 3)
    assert len(want[0]["live_seqs"]) == 1 and want[0]["steps"] == MAX_STEPS + 1
    bs = BaselineBatchedBeamSearch(dec, 3)
    got = bs.search(feats.to(DEV), START, END, max_steps=MAX_STEPS, return_all=True)
    assert bs.last_stats["steps"] == MAX_STEPS + 1
    for i in range(3):
        _check(got[i], bs.last_live[i], want[i])


def test_one_beam_is_greedy():
    from capmi.beam import BaselineBatchedBeamSearch
    dec, p = BC.decoder(M, H, V, 48, DEV, fc_scale=60.0, end_bias=2.0, end_idx=END)
    feats = torch.stack([t(gen.uniform(48 + i, "feats", (M,), -1, 1)) for i in range(3)])
    bs = BaselineBatchedBeamSearch(dec, 1)
    got = bs.search(feats.to(DEV), START, END, max_steps=MAX_STEPS)
    for i in range(3):
        seq, _, ended = BC.greedy_loop(p, feats[i], START, END, MAX_STEPS, dtype=torch.float64)
        if ended:
            assert got[i] == (seq, [], True)
        else:
            assert got[i] == ([START, END], [], False) and bs.last_live[i][0] == [seq]


def test_caption_images_through_the_real_encoder():
    import gen_captions as G
    from models.encoder import Encoder
    from vocabulary import synthetic_vocab
    torch.manual_seed(5)
    dec, _ = BC.decoder(M, H, V, 48, DEV, fc_scale=60.0, end_bias=2.0, end_idx=END)
    enc = Encoder(M).to(DEV).eval()
    imgs = t(gen.images(7, 2, 64, 64), DEV)
    vocab = synthetic_vocab(V)
    out = G.baseline_caption_images_beam_search(DEV, types.SimpleNamespace(beam_size=3), imgs, enc, dec, vocab)
    assert len(out) == 2
    for seq, alphas, ok in out:
        assert seq[0] == START and all(0 <= w < V for w in seq) and alphas == [] and isinstance(ok, bool)
        assert (seq[-1] == END) if ok else (seq == [START, END])
