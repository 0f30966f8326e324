"""Helper of the sampler tests (not a test): the contract of capmi_sample_step in fp64 (``pick_ref``), its
fp32 restatement on the CPU (``logp_fp32``: what fp32 arithmetic alone costs against fp64), and a forced-replay
loop for each decoder. The replay loops are built from the oracle.decoder_ref primitives (attention) and the
cell of tests/baseline_cases.py (baseline), as tests/beam_cases.py is: given the token sequence a row emitted
on the GPU they recompute every step's logits on the CPU along that prefix, so a draw that differs from the
CPU's never derails the steps after it."""
import torch
import torch.nn.functional as F

import baseline_cases as BLC
from oracle.decoder_ref import _lin, init_hidden_state, lstm_cell, soft_attention


def kept_mask(logits, top_k):
    """The kept set: the top_k largest raw fp32 logits by a stable descending sort (ties to the lower index);
    everything when top_k is 0 or >= V."""
    V = logits.numel()
    keep = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        idx = torch.sort(logits.float(), descending=True, stable=True)[1][:top_k]
        keep = torch.zeros(V, dtype=torch.bool)
        keep[idx] = True
    return keep


def pick_ref(logits, u, temperature, top_k):
    """logits (V,) fp32, u in [0, 1). Returns (token, logp, margin) computed in fp64. margin = min(u -
    cdf[token-1], cdf[token] - u) on the normalised CDF with cdf[-1] = 0: how far u is from drawing a
    neighbour (inf for the greedy pick, which does not use u)."""
    l = logits.double()
    lmax = l.max()
    if temperature == 0:
        tok = int((l == lmax).nonzero()[0])
        return tok, float(F.log_softmax(l, 0)[tok]), float("inf")
    keep = kept_mask(logits, top_k)
    w = torch.where(keep, torch.exp((l - lmax) / temperature), torch.zeros_like(l))
    S = w.sum()
    cdf = torch.cumsum(w, 0) / S
    hit = (cdf > u).nonzero()
    tok = int(hit[0]) if hit.numel() else int((w > 0).nonzero()[-1])
    below = float(cdf[tok - 1]) if tok > 0 else 0.0
    logp = float((l[tok] - lmax) / temperature - torch.log(S))
    return tok, logp, min(u - below, float(cdf[tok]) - u)


def logp_fp32(logits, tok, temperature, top_k):
    """logp of ``tok`` by the contract's formula in fp32 on the CPU, the sum taken sequentially in index order."""
    l = logits.float()
    lmax = l.max()
    keep = kept_mask(logits, top_k)
    w = torch.where(keep, torch.exp((l - lmax) / torch.tensor(temperature, dtype=torch.float32)),
                    torch.zeros_like(l))
    S = torch.cumsum(w, 0)[-1]
    return float((l[tok] - lmax) / torch.tensor(temperature, dtype=torch.float32) - torch.log(S))


@torch.no_grad()
def attention_replay(p, encoder_out, start_idx, tokens, dtype=torch.float64):
    """encoder_out (1, S, S, E) of one image, ``tokens`` the words one row emitted. Returns (logits (n, V),
    alphas (n, P)) of the n = len(tokens) steps whose inputs are start, tokens[0], ..., tokens[n-2]."""
    p = {n: v.to(dtype) if v.is_floating_point() else v for n, v in p.items()}
    E = encoder_out.size(-1)
    enc = encoder_out.to(dtype).view(1, -1, E)
    h, c = init_hidden_state(p, enc)
    prev = [start_idx] + list(tokens[:-1])
    logits, alphas = [], []
    for w in prev:
        emb = F.embedding(torch.LongTensor([w]), p["embedding.weight"])
        awe, alpha = soft_attention(p, enc, h)
        awe = torch.sigmoid(_lin(h, p, "f_beta")) * awe
        h, c = lstm_cell(torch.cat([emb.to(dtype), awe], dim=1), h, c, p)
        logits.append(_lin(h, p, "fc")[0])
        alphas.append(alpha[0])
    return torch.stack(logits), torch.stack(alphas)


@torch.no_grad()
def baseline_replay(p, feat, start_idx, tokens, dtype=torch.float64):
    """feat (M,) of one image. The baseline recurrence of capmi.beam.BaselineBatchedBeamSearch along ``tokens``:
    the image feature from a zero state, then h, c = LSTM(embedding(prev), (h, c)), logits = linear(h).
    Returns logits (n, V)."""
    q = {k: v.to(dtype) for k, v in p.items()}
    H = q["lstm.weight_hh_l0"].shape[1]
    z = torch.zeros(1, H, dtype=dtype)
    h, c = BLC.lstm_cell(q, feat.to(dtype).view(1, -1), z, z)
    logits = []
    for w in [start_idx] + list(tokens[:-1]):
        h, c = BLC.lstm_cell(q, q["embedding.weight"][w].view(1, -1), h, c)
        logits.append(F.linear(h, q["linear.weight"], q["linear.bias"])[0])
    return torch.stack(logits)
