"""Helper of the batched beam-search tests (not a test): a CPU beam loop built only from the
oracle.decoder_ref primitives, which also reports what oracle.beam_ref.beam_search does not return:
the beams still live at the stop and the selection margin. oracle.beam_ref stays the authority:
tests/test_beam_cases_cpu.py pins this loop to it on the three beam_search_* goldens."""
import torch
import torch.nn.functional as F

import gen
from helpers import make_decoder, t
from oracle.decoder_ref import _lin, init_hidden_state, lstm_cell, soft_attention


@torch.no_grad()
def beam_loop(p, encoder_out, k, start_idx, end_idx, max_steps=50, dtype=torch.float32):
    """encoder_out (1, S, S, E) of one image; the steps of oracle.beam_ref.beam_search in ``dtype``.
    Returns a dict: seq / alphas / ok (the oracle's return), done_seqs / done_scores (every finished
    beam in the order it finished), live_seqs / live_scores (the beams still live at the stop), steps,
    and margin = the smallest gap between adjacent values among the top s+1 candidates of any step
    (how far the selection, s beams and their order, is from changing)."""
    p = {n: v.to(dtype) if v.is_floating_point() else v for n, v in p.items()}
    side, E = encoder_out.size(1), encoder_out.size(-1)
    enc = encoder_out.to(dtype).view(1, -1, E)
    P = enc.size(1)
    enc = enc.expand(k, P, E)
    V = p["fc.weight"].shape[0]
    prev = torch.LongTensor([[start_idx]] * k)
    seqs = torch.LongTensor([[start_idx]] * k)
    top = torch.zeros(k, 1, dtype=dtype)
    seq_alpha = torch.ones(k, 1, side, side, dtype=dtype)
    done_seqs, done_alpha, done_scores = [], [], []
    margin = float("inf")
    step = 1
    h, c = init_hidden_state(p, enc)
    while True:
        emb = F.embedding(prev, p["embedding.weight"]).squeeze(1)
        awe, alpha = soft_attention(p, enc, h)
        alpha = alpha.view(-1, side, side).unsqueeze(1)
        awe = torch.sigmoid(_lin(h, p, "f_beta")) * awe
        x = torch.cat([emb.double(), awe.double()], dim=1)
        h, c = lstm_cell(x.to(dtype), h.to(dtype), c.to(dtype), p)
        scores = F.log_softmax(_lin(h, p, "fc"), dim=1)
        scores = top.expand_as(scores) + scores
        cand = scores[0] if step == 1 else scores.view(-1)
        top_s, top_w = cand.topk(k, 0, True, True)
        more = cand.topk(min(k + 1, cand.numel()), 0, True, True)[0].double()
        if more.numel() > 1:
            margin = min(margin, float((more[:-1] - more[1:]).min()))
        prev_i = top_w // V
        next_w = top_w % V
        seqs = torch.cat([seqs[prev_i], next_w.unsqueeze(1)], dim=1)
        seq_alpha = torch.cat([seq_alpha[prev_i], alpha[prev_i]], dim=1)
        inc = [i for i, w in enumerate(next_w) if w != end_idx]
        com = list(set(range(len(next_w))) - set(inc))
        if len(com) > 0:
            done_seqs.extend(seqs[com].tolist())
            done_alpha.extend(seq_alpha[com].tolist())
            done_scores.extend(float(v) for v in top_s[com])
        k -= len(com)
        seqs = seqs[inc]
        top = top_s[inc].unsqueeze(1)
        if k == 0:
            break
        seq_alpha = seq_alpha[inc]
        enc = enc[prev_i[inc]]
        h = h[prev_i[inc]]
        c = c[prev_i[inc]]
        prev = next_w[inc].unsqueeze(1)
        if step > max_steps:
            break
        step += 1
    out = dict(done_seqs=done_seqs, done_scores=done_scores, live_seqs=seqs.tolist(),
               live_scores=[float(v) for v in top.view(-1)], steps=step, margin=margin)
    if not done_seqs:
        out.update(seq=[start_idx, end_idx], alphas=[], ok=False)
    else:
        best = done_scores.index(max(done_scores))
        out.update(seq=done_seqs[best], alphas=done_alpha[best], ok=True)
    return out


def golden_params(fx):
    """Oracle parameters of a beam_search_* golden (fc scaled, <end> bias raised as it was generated)."""
    m = fx["meta"]
    p = {n: t(v) for n, v in gen.decoder_params(m["seed"], m["A"], m["D"], m["M"], m["V"]).items()}
    return tune_params(p, float(fx["fc_scale"]), float(fx["end_bias"]), m["end"])


def tune_params(p, fc_scale, end_bias, end_idx):
    p = dict(p)
    p["fc.weight"] = p["fc.weight"] * fc_scale
    p["fc.bias"] = p["fc.bias"].clone()
    p["fc.bias"][end_idx] += end_bias
    return p


def tuned_decoder(A, D, M, V, seed, fc_scale, end_bias, end_idx, device):
    """(capmi decoder on ``device``, oracle parameter dict), both with fc.weight * fc_scale and
    fc.bias[<end>] += end_bias."""
    dec, p = make_decoder(A, D, M, V, seed, device)
    dec.eval()
    with torch.no_grad():
        dec.fc.weight.mul_(fc_scale)
        dec.fc.bias[end_idx] += end_bias
    return dec, tune_params(p, fc_scale, end_bias, end_idx)


def features(seeds):
    """(B, 14, 14, 2048) features, image b = gen.encoder_features(seeds[b], 1)."""
    return torch.cat([t(gen.encoder_features(s, 1)).view(1, 14, 14, 2048) for s in seeds], 0)
