"""Helper of the baseline (LSTM) captioner's inference tests (not a test): the tiny seeded decoder, the fp64
oracle of one caption evaluated alone (reference models/baseline.py:267-374), the row contract of
capmi_eval_rows_at restated with its offset, and a CPU beam loop with the semantics of
capmi.beam.BaselineBatchedBeamSearch. Everything is plain torch / numpy written from the definitions."""
import numpy as np
import torch
import torch.nn.functional as F

import eval_cases as EC
import gen
from helpers import t

SHAPES = lambda M, H, V: {  # noqa: E731
    "embedding.weight": (V, M), "lstm.weight_ih_l0": (4 * H, M), "lstm.weight_hh_l0": (4 * H, H),
    "lstm.bias_ih_l0": (4 * H,), "lstm.bias_hh_l0": (4 * H,), "linear.weight": (V, H), "linear.bias": (V,)}


def params(M, H, V, seed):
    """The weights of tests/test_gpu_baseline.py::_decoder: gen.uniform(seed, name, shape, -0.2, 0.2)."""
    return {k: t(gen.uniform(seed, k, s, -0.2, 0.2)) for k, s in SHAPES(M, H, V).items()}


def decoder(M, H, V, seed, device, fc_scale=1.0, end_bias=0.0, end_idx=None):
    """(BaselineDecoder on ``device`` in eval mode, its parameter dict), linear.weight * fc_scale and
    linear.bias[end_idx] += end_bias in both."""
    from models.baseline import BaselineDecoder, BaselineDecoderParams
    prm = BaselineDecoderParams()
    prm.embed_size, prm.hidden_size, prm.vocab_size = M, H, V
    dec = BaselineDecoder(prm)
    p = params(M, H, V, seed)
    p["linear.weight"] = p["linear.weight"] * fc_scale
    if end_idx is not None:
        p["linear.bias"] = p["linear.bias"].clone()
        p["linear.bias"][end_idx] += end_bias
    dec.load_state_dict(p)
    return dec.to(device).eval(), p


def lstm_cell(p, x, h, c):
    """torch.nn.LSTM's cell, gate order i,f,g,o, in the dtype of its inputs."""
    g = x @ p["lstm.weight_ih_l0"].T + p["lstm.bias_ih_l0"] + h @ p["lstm.weight_hh_l0"].T + p["lstm.bias_hh_l0"]
    i, f, gg, o = g.chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def _cast(p, dtype):
    return {k: v.to(dtype) for k, v in p.items()}


def rows_ref(logits, caps, lens, tgt_off):
    """eval_cases.rows_ref with the target of row (b, t) at caps[b][t + tgt_off]."""
    caps = np.asarray(caps)
    shifted = np.zeros((caps.shape[0], logits.shape[1] + 1), np.int64)
    shifted[:, 1:] = caps[:, tgt_off:tgt_off + logits.shape[1]]
    return EC.rows_ref(logits, shifted, lens)


def oracle_caption(p, feat, cap, dtype=torch.float64):
    """feat (M,), cap 1-D int64 START..END of its own length n. Step 0 is fed the feature and scored against
    cap[0], step t embedding(cap[t-1]) against cap[t]; loss = the CE mean over the n rows.
    Returns dict: logits (n, V) numpy fp64, loss, pred / rank (n,), gap (n,) = top-1 minus top-2 logit,
    margin (n,) = the least |x[tgt] - x[v]|, v != tgt."""
    q = _cast(p, dtype)
    n = cap.numel()
    x = torch.cat([feat.to(dtype).view(1, -1), F.embedding(cap[:-1], q["embedding.weight"])], 0)
    h = torch.zeros(1, q["lstm.weight_hh_l0"].shape[1], dtype=dtype)
    c = torch.zeros_like(h)
    hs = []
    for s in range(n):
        h, c = lstm_cell(q, x[s:s + 1], h, c)
        hs.append(h)
    logits = F.linear(torch.cat(hs, 0), q["linear.weight"], q["linear.bias"]).double().numpy()
    loss_rows, pred, rank = rows_ref(logits[None], cap.view(1, -1).numpy(), [n], 0)
    top2 = np.sort(logits, axis=1)[:, -2:]
    tgt = cap.numpy()
    d = np.abs(logits - logits[np.arange(n), tgt][:, None])
    d[np.arange(n), tgt] = np.inf
    return dict(logits=logits, loss=float(loss_rows[0].sum() / n), pred=pred[0], rank=rank[0],
                gap=top2[:, 1] - top2[:, 0], margin=d.min(axis=1), n=n)


# 7 captions, 41 rows, not sorted, 7 % 4 != 0 (the attention model's E2E lengths)
E2E = dict(M=16, H=24, V=50, lengths=[5, 8, 3, 6, 4, 8, 7], batch_size=4)


def e2e_inputs(seed):
    """[(feature (M,), caption (n,) int64)] of the end-to-end case."""
    lengths = E2E["lengths"]
    caps = gen.captions(seed, len(lengths), max(lengths), E2E["V"], lengths=lengths)
    return [(t(gen.uniform(seed + i, "feats", (E2E["M"],), -1, 1)), t(caps[i, :n].copy()))
            for i, n in enumerate(lengths)]


class ListDataset(list):
    """Items (feature, caption) with the ``vocab`` the evaluators read off their dataset."""

    def __init__(self, items, V):
        from vocabulary import synthetic_vocab
        super().__init__(items)
        self.vocab = synthetic_vocab(V)


class IdentityEncoder:
    """Features stand in for images."""

    def __call__(self, x):
        return x

    def eval(self):
        return self


@torch.no_grad()
def beam_loop(p, feat, k, start_idx, end_idx, max_steps=50, dtype=torch.float32):
    """The baseline beam search of one image on the CPU in ``dtype``: the state after the image feature is the
    initial (h, c) of all k beams, sequences start as [START] with score 0, then the loop of
    tests/beam_cases.py::beam_loop with h, c = LSTM(embedding(prev), (h, c)), logits = linear(h).
    Returns dict: seq / ok, done_seqs / done_scores (in finishing order), live_seqs / live_scores (at the stop),
    steps, margin (the smallest gap between adjacent values among the top s+1 candidates of any step)."""
    q = _cast(p, dtype)
    V = q["linear.weight"].shape[0]
    H = q["lstm.weight_hh_l0"].shape[1]
    h, c = lstm_cell(q, feat.to(dtype).view(1, -1), torch.zeros(1, H, dtype=dtype), torch.zeros(1, H, dtype=dtype))
    h, c = h.expand(k, H).clone(), c.expand(k, H).clone()
    prev = torch.LongTensor([start_idx] * k)
    seqs = torch.LongTensor([[start_idx]] * k)
    top = torch.zeros(k, 1, dtype=dtype)
    done_seqs, done_scores = [], []
    margin = float("inf")
    step = 1
    while True:
        h, c = lstm_cell(q, F.embedding(prev, q["embedding.weight"]), h, c)
        scores = F.log_softmax(F.linear(h, q["linear.weight"], q["linear.bias"]), dim=1)
        scores = top.expand_as(scores) + scores
        cand = scores[0] if step == 1 else scores.view(-1)
        top_s, top_w = cand.topk(k, 0, True, True)
        more = cand.topk(min(k + 1, cand.numel()), 0, True, True)[0].double()
        if more.numel() > 1:
            margin = min(margin, float((more[:-1] - more[1:]).min()))
        prev_i = top_w // V
        next_w = top_w % V
        seqs = torch.cat([seqs[prev_i], next_w.unsqueeze(1)], dim=1)
        inc = [i for i, w in enumerate(next_w) if w != end_idx]
        com = sorted(set(range(len(next_w))) - set(inc))
        if com:
            done_seqs.extend(seqs[com].tolist())
            done_scores.extend(float(v) for v in top_s[com])
        k -= len(com)
        seqs = seqs[inc]
        top = top_s[inc].unsqueeze(1)
        if k == 0:
            break
        h, c = h[prev_i[inc]], c[prev_i[inc]]
        prev = next_w[inc]
        if step > max_steps:
            break
        step += 1
    out = dict(done_seqs=done_seqs, done_scores=done_scores, live_seqs=seqs.tolist(),
               live_scores=[float(v) for v in top.view(-1)], steps=step, margin=margin)
    if not done_seqs:
        out.update(seq=[start_idx, end_idx], ok=False)
    else:
        out.update(seq=done_seqs[done_scores.index(max(done_scores))], ok=True)
    return out


@torch.no_grad()
def greedy_loop(p, feat, start_idx, end_idx, max_steps=50, dtype=torch.float32):
    """Free-running greedy decode (what a beam of 1 is): (sequence, summed log-probability, ended)."""
    q = _cast(p, dtype)
    H = q["lstm.weight_hh_l0"].shape[1]
    h, c = lstm_cell(q, feat.to(dtype).view(1, -1), torch.zeros(1, H, dtype=dtype), torch.zeros(1, H, dtype=dtype))
    seq, score, prev = [start_idx], 0.0, start_idx
    for _ in range(max_steps + 1):
        h, c = lstm_cell(q, q["embedding.weight"][prev].view(1, -1), h, c)
        lp = F.log_softmax(F.linear(h, q["linear.weight"], q["linear.bias"]), dim=1)[0]
        prev = int(lp.argmax())
        score += float(lp[prev])
        seq.append(prev)
        if prev == end_idx:
            return seq, score, True
    return seq, score, False
