"""GPU: batched beam search (capmi.beam.BatchedBeamSearch; csrc/beam.hip) -- the three entry points
against fp64 / the oracle on the CPU, then whole searches per image against oracle.beam_ref (the
authority) and tests/beam_cases.py (live beams, selection margins), the reference's own goldens at
B = 1 and inside a batch, the step / host-sync accounting and the public surface."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import beam_cases as BC
import gen
from helpers import assert_close, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = dict(dtype=torch.int32, device=DEV)
CANARY = -7.0


# ---------------------------------------------------------------------------------------------
# 1. capmi_beam_select
# ---------------------------------------------------------------------------------------------
def _select(logits, scores, live, first, B, k, V):
    from capmi import kernels as K
    parent = torch.full((B, k), int(CANARY), **I32)
    word = torch.full((B, k), int(CANARY), **I32)
    top = torch.full((B, k), CANARY, device=DEV)
    cand_v = torch.empty(B * k * k, device=DEV)
    cand_w = torch.empty(B * k * k, **I32)
    K.beam_select(logits.to(DEV), scores.to(DEV), torch.tensor(live, **I32), first, B, k, V, cand_v, cand_w,
                  parent, word, top)
    torch.cuda.synchronize()
    return parent.cpu(), word.cpu(), top.cpu()


def _select_ref(logits, scores, live, first, k, V):
    """Per image: stable descending sort of score + log_softmax in fp64 -> (flat indices, values, all values)."""
    lp = scores.double().unsqueeze(1) + F.log_softmax(logits.double(), dim=1)
    out = []
    for i, s in enumerate(live):
        rows = min(s, 1) if first else s
        cand = lp[i * k:i * k + rows].reshape(-1)
        v, idx = torch.sort(cand, descending=True, stable=True)
        out.append((idx, v))
    return out


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("V,k", [(50, 3), (120, 5), (8100, 5), (8100, 16), (7, 1)])
def test_beam_select_matches_fp64(V, k, first):
    B, live = 3, [k, 1, 0]
    g = torch.Generator().manual_seed(9000 + V + k)
    logits = 3.0 * torch.randn(B * k, V, generator=g)
    scores = -3.0 * torch.rand(B * k, generator=g)
    ref = _select_ref(logits, scores, live, first, k, V)
    parent, word, top = _select(logits, scores, live, first, B, k, V)
    for i, s in enumerate(live):
        idx, v = ref[i]
        if s:
            head = v[:min(s + 1, v.numel())]
            if head.numel() > 1:  # the test's own precondition: the fp64 order is not within fp32 rounding
                assert float((head[:-1] - head[1:]).min()) > 1e-4
            assert parent[i, :s].tolist() == (idx[:s] // V).tolist()
            assert word[i, :s].tolist() == (idx[:s] % V).tolist()
            print(f"V {V} k {k} first {first} image {i}: max |top - fp64| "
                  f"{float((top[i, :s].double() - v[:s]).abs().max()):.3g}")
            assert_close(top[i, :s], v[:s], 1e-6, 1e-6, "beam scores")
        assert (parent[i, s:] == int(CANARY)).all() and (word[i, s:] == int(CANARY)).all()
        assert (top[i, s:] == CANARY).all()


def test_beam_select_exact_ties_take_the_lower_flat_index():
    V, k, B = 50, 3, 2
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(B * k, V, generator=g)
    logits[0, 4] = logits[0, 10] = 6.0       # a repeated column inside a row
    logits[1] = logits[0]                    # two identical rows with identical beam scores
    logits[3] = logits[5] = logits[4]        # image 1: three identical rows, no repeated column
    scores = torch.tensor([-1.5, -1.5, -9.0, -2.0, -2.0, -2.0])
    parent, word, top = _select(logits, scores, [3, 3], 0, B, k, V)
    assert parent[0].tolist() == [0, 0, 1] and word[0].tolist() == [4, 10, 4]
    assert top[0, 0] == top[0, 1] == top[0, 2]
    w = int(logits[4].argmax())
    assert parent[1].tolist() == [0, 1, 2] and word[1].tolist() == [w, w, w]
    assert top[1, 0] == top[1, 1] == top[1, 2]
    ref = _select_ref(logits, scores, [3, 3], 0, k, V)
    for i in range(B):
        assert (ref[i][0][:3] // V).tolist() == parent[i].tolist() and (ref[i][0][:3] % V).tolist() == word[i].tolist()
    # first step: row 0 alone, so the repeated column gives the only tie
    parent, word, top = _select(logits, scores, [3, 3], 1, B, k, V)
    assert parent[0].tolist() == [0, 0, 0] and word[0].tolist()[:2] == [4, 10] and top[0, 0] == top[0, 1]


# ---------------------------------------------------------------------------------------------
# 2. capmi_beam_att_fwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,k,P,E,A,slabs", [(1, 1, 196, 2048, 32, 1), (3, 5, 196, 2048, 64, 2),
                                             (2, 3, 49, 2048, 512, 1)])
def test_beam_att_fwd_matches_oracle(B, k, P, E, A, slabs):
    """Features once per image on the device; the oracle (fp64) on features repeated per beam. Dead rows
    (at or past live[i]) are never written: their canaries must survive."""
    from capmi import kernels as K
    from oracle.decoder_ref import _lin, soft_attention
    D, M, R = 32, 16, B * k
    live = [k, 2, 0][:B] if k >= 2 else [k]
    p = {n: t(v) for n, v in gen.decoder_params(300 + A, A, D, M, 50).items()}
    enc = t(gen.encoder_features(300 + P, B, P=P)).reshape(B, P, E)
    h = torch.randn(R, D, generator=torch.Generator().manual_seed(5)) * 0.5
    att_enc = _lin(enc, p, "attention.enc_att")
    W_da, W_fb = p["attention.dec_att.weight"], p["f_beta.weight"]
    cut = [0, D] if slabs == 1 else [0, D // 2, D]
    dec_part = torch.stack([h[:, a:b] @ W_da[:, a:b].t() for a, b in zip(cut, cut[1:])])   # (S, R, A)
    gate_part = torch.stack([h[:, a:b] @ W_fb[:, a:b].t() for a, b in zip(cut, cut[1:])])  # (S, R, E)
    X = M + E
    can = lambda *s: torch.full(s, CANARY, device=DEV)  # noqa: E731
    alpha, awe, gate, x, e_ws = can(R, P), can(R, E), can(R, E), can(R, X), can(R, P)
    K.beam_att_fwd(enc.to(DEV), att_enc.to(DEV), dec_part.to(DEV), slabs, R * A,
                   p["attention.dec_att.bias"].to(DEV), p["attention.full_att.weight"].view(-1).to(DEV),
                   p["attention.full_att.bias"].to(DEV), gate_part.to(DEV), slabs, R * E, p["f_beta.bias"].to(DEV),
                   torch.tensor(live, **I32), B, k, P, A, E, e_ws, alpha_out=alpha, awe_out=awe, gate_out=gate,
                   x_out=x[:, M:], ld_x=X)
    torch.cuda.synchronize()
    p64 = {n: v.double() for n, v in p.items()}
    rawe, ralpha = soft_attention(p64, enc.double().repeat_interleave(k, 0), h.double())
    rgate = torch.sigmoid(_lin(h.double(), p64, "f_beta"))
    rows = [i * k + j for i in range(B) for j in range(live[i])]
    dead = [r for r in range(R) if r not in rows]
    assert_close(alpha[rows], ralpha[rows], 0.0, 1e-5, "alpha")
    assert_close(awe[rows], rawe[rows], 1e-4, 0.0, "context")
    assert_close(gate[rows], rgate[rows], 1e-4, 0.0, "gate")
    assert_close(x[rows][:, M:], (rgate * rawe)[rows], 1e-4, 0.0, "gated context")
    assert (x[:, :M] == CANARY).all()
    for buf in (alpha, awe, gate, x):
        assert (buf[dead] == CANARY).all()


# ---------------------------------------------------------------------------------------------
# 3. whole searches, per image against the oracle
# ---------------------------------------------------------------------------------------------
DEC = (64, 48, 32, 120, 62)   # make_decoder(A, D, M, V, seed)
START, END = 117, 118         # synthetic_vocab(120): <start> = V-3, <end> = V-2
SETTINGS = {"mixed": (2.0, 0.8, (62, 162, 262, 462)),            # finish at different steps, one beam to the cap
            "all_finish": (1.0, 0.5, (62, 162, 262, 362, 462, 562))}  # every beam finished by step 3


@functools.lru_cache(maxsize=None)
def _oracle(setting, max_steps=14):
    from oracle.beam_ref import beam_search
    fc_scale, end_bias, seeds = SETTINGS[setting]
    dec, p = BC.tuned_decoder(*DEC, fc_scale, end_bias, END, DEV)
    feats = BC.features(seeds)
    ref = [beam_search(p, feats[i:i + 1], 5, START, END, max_steps=max_steps, return_all=True)
           for i in range(len(seeds))]
    helper = [BC.beam_loop(p, feats[i:i + 1], 5, START, END, max_steps=max_steps) for i in range(len(seeds))]
    return dec, feats, ref, helper


def _check_image(got, live, ref, helper, what):
    seq, alphas, ok, (done, scores) = got
    rseq, ralphas, rok, (rdone, rscores) = ref
    assert helper["margin"] >= 1e-3, f"{what}: oracle selection margin {helper['margin']:.3g}"
    assert ok == rok and seq == rseq, what
    assert done == rdone, what
    np.testing.assert_allclose(scores, rscores, rtol=1e-4, atol=1e-5, err_msg=what)
    assert np.array(alphas).shape == np.array(ralphas).shape
    np.testing.assert_allclose(np.array(alphas), np.array(ralphas), rtol=0, atol=1e-5, err_msg=what)
    assert live[0] == helper["live_seqs"], what
    np.testing.assert_allclose(live[1], helper["live_scores"], rtol=1e-4, atol=1e-5, err_msg=what)


@pytest.mark.parametrize("setting", ["mixed", "all_finish"])
def test_batched_search_matches_oracle_per_image(setting):
    from capmi.beam import BatchedBeamSearch
    dec, feats, ref, helper = _oracle(setting)
    bs = BatchedBeamSearch(dec, 5)
    got = bs.search(feats.to(DEV), START, END, max_steps=14, return_all=True)
    assert len(got) == feats.size(0)
    for i in range(feats.size(0)):
        _check_image(got[i], bs.last_live[i], ref[i], helper[i], f"{setting} image {i}")
    lens = [sorted(len(s) for s in r[3][0]) for r in ref]
    if setting == "mixed":  # what the case is there for: images of one batch stop at different steps
        assert lens[:3] == [[2, 3, 3, 4]] * 3 and len(lens[3]) == 5 and max(lens[3]) <= 4
        assert [len(h["live_seqs"]) for h in helper] == [1, 1, 1, 0]
    else:
        assert lens == [[2, 3, 3, 4, 4]] * len(lens) and not any(h["live_seqs"] for h in helper)
    no_alpha = bs.search(feats.to(DEV), START, END, max_steps=14, return_alphas=False)
    assert [(r[0], r[2]) for r in no_alpha] == [(r[0], r[2]) for r in got] and all(r[1] == [] for r in no_alpha)


# ---------------------------------------------------------------------------------------------
# 4. the reference's own goldens, alone and inside a batch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("tag", ["small", "k5", "noend"])
def test_goldens_through_the_batched_search(golden, tag, B):
    from capmi.beam import BatchedBeamSearch
    fx = golden(f"beam_search_{tag}")
    m = fx["meta"]
    dec, _ = BC.tuned_decoder(m["A"], m["D"], m["M"], m["V"], m["seed"], float(fx["fc_scale"]), float(fx["end_bias"]),
                              m["end"], DEV)
    feats = BC.features([m["seed"] + 100 * b for b in range(B)])
    got = BatchedBeamSearch(dec, m["k"]).search(feats.to(DEV), m["start"], m["end"])
    assert len(got) == B
    seq, alphas, ok = got[0]
    assert bool(ok) == bool(fx["ok"]) and seq == fx["seq"].tolist()
    got_a = np.array(alphas, dtype=np.float32).reshape(fx["alphas"].shape)
    np.testing.assert_allclose(got_a, fx["alphas"], rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------------------------
# 5. step and host-sync accounting
# ---------------------------------------------------------------------------------------------
def test_never_ending_beams_run_to_the_cap_without_per_step_syncs(golden):
    from capmi.beam import BatchedBeamSearch
    fx = golden("beam_search_noend")
    m = fx["meta"]
    dec, p = BC.tuned_decoder(m["A"], m["D"], m["M"], m["V"], m["seed"], float(fx["fc_scale"]),
                              float(fx["end_bias"]), m["end"], DEV)
    feats = BC.features([63, 163])
    bs = BatchedBeamSearch(dec, m["k"])
    got = bs.search(feats.to(DEV), m["start"], m["end"], max_steps=14)
    assert got == [([m["start"], m["end"]], [], False)] * 2
    assert bs.last_stats["steps"] == 15 and bs.last_stats["host_syncs"] <= 3
    for i in range(2):
        helper = BC.beam_loop(p, feats[i:i + 1], m["k"], m["start"], m["end"], max_steps=14)
        assert helper["margin"] >= 1e-3 and helper["steps"] == 15
        assert bs.last_live[i][0] == helper["live_seqs"]
        np.testing.assert_allclose(bs.last_live[i][1], helper["live_scores"], rtol=1e-4, atol=1e-5)


def test_early_stop_when_every_image_has_finished():
    from capmi.beam import BatchedBeamSearch
    dec, feats, ref, helper = _oracle("all_finish")
    bs = BatchedBeamSearch(dec, 5)
    got = bs.search(feats.to(DEV), START, END, max_steps=14, sync_every=1)
    assert bs.last_stats["steps"] == 3 == max(h["steps"] for h in helper)
    assert [r[0] for r in got] == [r[0] for r in ref]


# ---------------------------------------------------------------------------------------------
# 6. surface and limits
# ---------------------------------------------------------------------------------------------
def test_caption_images_beam_search_surface():
    """Identity "encoder" over stacked features. The all-finish setting: every beam has ended by step 3, so
    the surface's default step cap gives what test 3 checked at max_steps = 14."""
    from gen_captions import caption_images_beam_search
    from vocabulary import synthetic_vocab
    dec, feats, ref, helper = _oracle("all_finish")
    got = caption_images_beam_search(DEV, types.SimpleNamespace(beam_size=5), feats.to(DEV), lambda imgs: imgs, dec,
                                     synthetic_vocab(DEC[3]))
    assert len(got) == feats.size(0) and all(len(r) == 3 for r in got)
    for i, (seq, alphas, ok) in enumerate(got):
        assert helper[i]["margin"] >= 1e-3
        assert (seq, ok) == (ref[i][0], ref[i][2])
        np.testing.assert_allclose(np.array(alphas), np.array(ref[i][1]), rtol=0, atol=1e-5)


def test_limits():
    from capmi.beam import BatchedBeamSearch
    dec, _ = BC.tuned_decoder(*DEC, 1.0, 0.0, END, DEV)
    for k in (0, 17):
        with pytest.raises(ValueError):
            BatchedBeamSearch(dec, k)
    dec.use_bert = True
    with pytest.raises(NotImplementedError):
        BatchedBeamSearch(dec, 5).search(BC.features([62]).to(DEV), START, END)
