"""Beam-search captioning on the capmi kernels.

Restates ``attention_caption_image_beam_search`` (gen_captions.py:16-131 of the reference): one
image, k beams treated as a batch of k, per step the soft attention, the f_beta gate, the
LSTMCell and the vocabulary projection, then log_softmax + top-k over the (beams x V) scores and
the bookkeeping of finished beams. The arithmetic of a step runs on the same HIP kernels as the
training forward (grouped h-GEMM, fused ReLU score, softmax + context + gate, LSTM pointwise);
``enc_att(encoder_out)`` is computed once per image (the reference recomputes it every step,
Q5). The selection logic (top-k over at most k*V scores, beam reordering) is a few tiny torch
ops on the device, as in the reference.

``BatchedBeamSearch`` runs the same algorithm for B images per call: the k beams of every image are
rows of one batch of B*k, the features stay once per image, and selection and bookkeeping are HIP
kernels (csrc/beam.hip), so a decode step is a fixed launch sequence without a host sync.

``BaselineBatchedBeamSearch`` is the same search for the baseline (LSTM) captioner: the step is one
capmi_lstm_step_fwd launch (csrc/baseline_step.hip), selection and bookkeeping are the same two kernels.
"""
import torch

from . import kernels as K
from ._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_NMAJOR_W as BW


class BeamSearch:
    def __init__(self, decoder, beam_size):
        self.dec = decoder
        self.k = int(beam_size)
        if self.k < 1:
            raise ValueError("beam_size must be >= 1")

    def _params(self):
        d = self.dec
        return dict(W_ea=d.attention.enc_att.weight, b_ea=d.attention.enc_att.bias,
                    W_da=d.attention.dec_att.weight, b_da=d.attention.dec_att.bias,
                    wf=d.attention.full_att.weight.view(-1), bf=d.attention.full_att.bias,
                    W_ih=d.decode_step.weight_ih, W_hh=d.decode_step.weight_hh,
                    b_ih=d.decode_step.bias_ih, b_hh=d.decode_step.bias_hh,
                    W_h=d.h_lin.weight, b_h=d.h_lin.bias, W_c=d.c_lin.weight, b_c=d.c_lin.bias,
                    W_fb=d.f_beta.weight, b_fb=d.f_beta.bias, W_fc=d.fc.weight, b_fc=d.fc.bias,
                    emb=d.embedding.weight)

    @torch.no_grad()
    def search(self, encoder_out, start_idx, end_idx, max_steps=50, return_all=False):
        """encoder_out: (1, 14, 14, E) or (1, P, E) features of ONE image. Returns
        (sequence list[int], alphas list (steps, P), finished bool) like the reference
        (failure: ([start, end], [], False)); with ``return_all`` also (every finished sequence,
        their scores)."""
        if self.dec.use_bert:
            raise NotImplementedError("beam search with BERT features (the reference notes it fails too)")
        p = self._params()
        dev = encoder_out.device
        E = encoder_out.size(-1)
        enc1 = encoder_out.reshape(1, -1, E).contiguous().float()
        P = enc1.size(1)
        k = self.k
        A, D = p["W_ea"].shape[0], p["W_hh"].shape[1]
        M, V = p["emb"].shape[1], p["W_fc"].shape[0]
        X = M + E
        f = dict(device=dev, dtype=torch.float32)
        # per image: att_enc once, init state (gen_captions.py:57; models/attention.py:151-164)
        att1 = torch.empty(P, A, **f)
        K.gemm(K.problem(P, A, E, enc1, E, p["W_ea"], E, att1, A, bias=p["b_ea"]), AK, BW, K.TILE_64)
        mean = torch.empty(1, E, **f)
        K.mean_rows(enc1, 1, P, E, mean)
        h = torch.empty(k, D, **f)
        c = torch.empty(k, D, **f)
        K.gemm([K.problem(1, D, E, mean, E, p["W_h"], E, h, D, bias=p["b_h"]),
                K.problem(1, D, E, mean, E, p["W_c"], E, c, D, bias=p["b_c"])], AK, BW, K.TILE_64)
        h[1:] = h[0]
        c[1:] = c[0]
        # beams of one image share its features: expanded once
        encK = enc1.expand(k, P, E).contiguous()
        attK = att1.unsqueeze(0).expand(k, P, A).contiguous()
        xin = torch.empty(k, X, **f)
        p_ad, p_gate = torch.empty(k, A, **f), torch.empty(k, E, **f)
        p_hh, p_x = torch.empty(k, 4 * D, **f), torch.empty(k, 4 * D, **f)
        e = torch.empty(k, P, **f)
        alpha, awe, gate = torch.empty(k, P, **f), torch.empty(k, E, **f), torch.empty(k, E, **f)
        act, h2, c2 = torch.empty(k, 4 * D, **f), torch.empty(k, D, **f), torch.empty(k, D, **f)
        scores = torch.empty(k, V, **f)

        prev = torch.full((k, 1), start_idx, dtype=torch.int64, device=dev)
        seqs = prev.clone()
        top = torch.zeros(k, 1, **f)
        seq_alpha = torch.ones(k, 1, P, **f)
        done_seqs, done_alpha, done_scores = [], [], []
        s, step, ended = k, 1, False
        while True:
            # embeddings (gen_captions.py:64) -> x[:, :M]; attention + gate -> x[:, M:]
            K.embed_gather(p["emb"], prev, s, 1, 1, xin, X)
            K.gemm([K.problem(s, A, D, h, D, p["W_da"], D, p_ad, A),
                    K.problem(s, E, D, h, D, p["W_fb"], D, p_gate, E),
                    K.problem(s, 4 * D, D, h, D, p["W_hh"], D, p_hh, 4 * D)], AK, BW, K.TILE_64)
            K.att_score_fwd(attK, p_ad, 1, 0, p["b_da"], p["wf"], p["bf"], s, P, A, e)
            K.att_softmax_ctx_fwd(e, encK, s, P, E, s, alpha, P, awe, p_gate, 1, 0, p["b_fb"], gate,
                                  xin[:, M:], X)
            K.gemm(K.problem(s, 4 * D, X, xin, X, p["W_ih"], X, p_x, 4 * D, bias=p["b_ih"], bias2=p["b_hh"]),
                   AK, BW, K.TILE_64)
            K.lstm_cell_fwd(p_x, 1, 0, None, p_hh, 1, 0, c, s, D, h2, c2, act)
            K.gemm(K.problem(s, V, D, h2, D, p["W_fc"], D, scores, V, bias=p["b_fc"]), AK, BW, K.TILE_64)
            # selection (gen_captions.py:74-117)
            lp = torch.log_softmax(scores[:s], dim=1) + top.expand(s, V)
            if step == 1:
                top_s, top_w = lp[0].topk(s, 0, True, True)
            else:
                top_s, top_w = lp.view(-1).topk(s, 0, True, True)
            prev_i = torch.div(top_w, V, rounding_mode="floor")
            next_w = top_w % V
            seqs = torch.cat([seqs[prev_i], next_w.unsqueeze(1)], dim=1)
            seq_alpha = torch.cat([seq_alpha[prev_i], alpha[:s][prev_i].unsqueeze(1)], dim=1)
            nw = next_w.tolist()
            inc = [i for i, w in enumerate(nw) if w != end_idx]
            com = sorted(set(range(len(nw))) - set(inc))
            if com:
                ended = True
                done_seqs.extend(seqs[com].tolist())
                done_alpha.extend(seq_alpha[com].tolist())
                done_scores.extend(top_s[com].tolist())
            s -= len(com)
            if s == 0:
                break
            seqs, seq_alpha = seqs[inc], seq_alpha[inc]
            top = top_s[inc].unsqueeze(1)
            sel = prev_i[inc]
            h[:s] = h2[:len(nw)][sel]
            c[:s] = c2[:len(nw)][sel]
            prev = next_w[inc].unsqueeze(1).contiguous()
            if step > max_steps:
                break
            step += 1
        extra = ((done_seqs, done_scores),) if return_all else ()
        if not ended:
            return ([start_idx, end_idx], [], False) + extra
        best = done_scores.index(max(done_scores))
        al = done_alpha[best]
        if encoder_out.dim() == 4:  # (steps+1, 14, 14) like the reference's seqs_alpha
            hh, ww = encoder_out.size(1), encoder_out.size(2)
            al = [[row[i * ww:(i + 1) * ww] for i in range(hh)] for row in al]
        return (done_seqs[best], al, True) + extra


class BatchedBeamSearch(BeamSearch):
    """Beam search over B images per call. The beams of image i are rows i*k .. i*k+k-1 of every per-step
    tensor, its live ones compacted to the front. Features and ``enc_att`` features exist once per image
    (``capmi_beam_att_fwd`` serves the k rows of an image from one load; nothing is expanded k-fold).
    Selection and bookkeeping are two device entry points (``capmi_beam_select``, ``capmi_beam_advance``),
    so a step needs no host sync: the host reads the device count of images that still have live beams
    every ``sync_every`` steps only, and rebuilds the sequences after the loop from the back-pointers."""

    def __init__(self, decoder, beam_size):
        super().__init__(decoder, beam_size)
        if self.k > 16:
            raise ValueError("beam_size must be <= 16")
        self.last_stats = None
        self.last_live = None

    @torch.no_grad()
    def search(self, encoder_out, start_idx, end_idx, max_steps=50, return_all=False, return_alphas=True,
               sync_every=8):
        """encoder_out: (B, S, S, E) or (B, P, E). Returns a list of B tuples, each the single-image
        method's: (sequence, alphas (steps+1, S, S) or (steps+1, P) nested lists, finished) [+ (finished
        sequences, their scores) with ``return_all``]; failure: ([start, end], [], False). Without
        ``return_alphas`` the alphas are []. ``last_stats`` = steps run and host syncs taken;
        ``last_live`` = per image (sequences, scores) of the beams still live at the stop."""
        if self.dec.use_bert:
            raise NotImplementedError("beam search with BERT features (the reference notes it fails too)")
        p = self._params()
        dev = encoder_out.device
        B, E = encoder_out.size(0), encoder_out.size(-1)
        enc = encoder_out.reshape(B, -1, E).contiguous().float()
        P, k = enc.size(1), self.k
        R = B * k
        A, D = p["W_ea"].shape[0], p["W_hh"].shape[1]
        M, V = p["emb"].shape[1], p["W_fc"].shape[0]
        X = M + E
        T = int(max_steps) + 1
        sync_every = max(1, int(sync_every))
        f = dict(device=dev, dtype=torch.float32)
        # per batch: att_enc and the initial state, once per image
        att_enc = torch.empty(B * P, A, **f)
        K.gemm(K.problem(B * P, A, E, enc, E, p["W_ea"], E, att_enc, A, bias=p["b_ea"]), AK, BW, K.TILE_64)
        mean = torch.empty(B, E, **f)
        K.mean_rows(enc, B, P, E, mean)
        h0, c0 = torch.empty(B, D, **f), torch.empty(B, D, **f)
        K.gemm([K.problem(B, D, E, mean, E, p["W_h"], E, h0, D, bias=p["b_h"]),
                K.problem(B, D, E, mean, E, p["W_c"], E, c0, D, bias=p["b_c"])], AK, BW, K.TILE_64)
        h = h0.repeat_interleave(k, 0).contiguous()
        c = c0.repeat_interleave(k, 0).contiguous()
        xin = torch.zeros(R, X, **f)
        p_ad, p_gate = torch.empty(R, A, **f), torch.empty(R, E, **f)
        p_hh, p_x = torch.empty(R, 4 * D, **f), torch.empty(R, 4 * D, **f)
        e_ws = torch.empty(R, P, **f)
        act, h2, c2 = torch.empty(R, 4 * D, **f), torch.empty(R, D, **f), torch.empty(R, D, **f)
        logits = torch.empty(R, V, **f)
        alphas = torch.zeros(T, R, P, **f) if return_alphas else None
        cand_v = torch.empty(R * k, **f)
        cand_w = torch.empty(R * k, dtype=torch.int32, device=dev)
        prev = torch.full((R,), start_idx, dtype=torch.int64, device=dev)
        # every small piece of beam state in one int32 buffer: one copy brings it to the host
        sizes = dict(bp=T * 3 * R, fin_count=B, fin_step=R, fin_slot=R, fin_score=R, live=B, scores=R,
                     images_live=1, parent=R, word=R, top=R)
        state = torch.zeros(sum(sizes.values()), dtype=torch.int32, device=dev)
        off, o = {}, 0
        for name, n in sizes.items():
            off[name] = (o, o + n)
            o += n

        def piece(buf, name, as_float=False):
            v = buf[off[name][0]:off[name][1]]
            return v.view(torch.float32) if as_float else v

        bp = piece(state, "bp").view(T, 3, R)
        live, images_live = piece(state, "live"), piece(state, "images_live")
        live.fill_(k)
        images_live.fill_(B)
        scores, top = piece(state, "scores", True), piece(state, "top", True)
        parent, word = piece(state, "parent"), piece(state, "word")
        fin_count, fin_step, fin_slot = piece(state, "fin_count"), piece(state, "fin_step"), piece(state, "fin_slot")
        fin_score = piece(state, "fin_score", True)

        steps = syncs = 0
        for t_ in range(T):
            K.embed_gather(p["emb"], prev, R, 1, 1, xin, X)
            K.gemm([K.problem(R, A, D, h, D, p["W_da"], D, p_ad, A),
                    K.problem(R, E, D, h, D, p["W_fb"], D, p_gate, E),
                    K.problem(R, 4 * D, D, h, D, p["W_hh"], D, p_hh, 4 * D)], AK, BW, K.TILE_64)
            K.beam_att_fwd(enc, att_enc, p_ad, 1, 0, p["b_da"], p["wf"], p["bf"], p_gate, 1, 0, p["b_fb"], live,
                           B, k, P, A, E, e_ws, alpha_out=alphas[t_] if return_alphas else None,
                           x_out=xin[:, M:], ld_x=X)
            K.gemm(K.problem(R, 4 * D, X, xin, X, p["W_ih"], X, p_x, 4 * D, bias=p["b_ih"], bias2=p["b_hh"]),
                   AK, BW, K.TILE_64)
            K.lstm_cell_fwd(p_x, 1, 0, None, p_hh, 1, 0, c, R, D, h2, c2, act)
            K.gemm(K.problem(R, V, D, h2, D, p["W_fc"], D, logits, V, bias=p["b_fc"]), AK, BW, K.TILE_64)
            K.beam_select(logits, scores, live, t_ == 0, B, k, V, cand_v, cand_w, parent, word, top)
            K.beam_advance(parent, word, top, live, B, k, D, end_idx, t_, h2, c2, h, c, prev, scores,
                           bp[t_, 0], bp[t_, 1], bp[t_, 2], fin_count, fin_step, fin_slot, fin_score, images_live)
            steps += 1
            if steps % sync_every == 0 and steps < T:
                syncs += 1
                if int(images_live.item()) == 0:
                    break
        host = state.cpu()
        syncs += 1
        bp_h = piece(host, "bp").view(T, 3, B, k).numpy()
        live_h, nfin = piece(host, "live").tolist(), piece(host, "fin_count").tolist()
        fstep, fslot = piece(host, "fin_step").view(B, k).tolist(), piece(host, "fin_slot").view(B, k).tolist()
        fscore = piece(host, "fin_score", True).view(B, k).tolist()
        scores_h = piece(host, "scores", True).view(B, k).tolist()

        def walk(i, t_, slot):
            """the beam selected at step t_ as slot: its words and, per step, the row whose alpha it took"""
            words, rows = [], []
            while True:
                row = int(bp_h[t_, 0, i, slot])
                words.append(int(bp_h[t_, 1, i, slot]))
                rows.append(t_ * R + i * k + row)
                if t_ == 0:
                    break
                t_ -= 1
                slot = int(bp_h[t_, 2, i, row])
            return [start_idx] + words[::-1], rows[::-1]

        results, paths, self.last_live = [], [], []
        for i in range(B):
            done = [walk(i, fstep[i][q], fslot[i][q]) for q in range(nfin[i])]
            dscores = fscore[i][:nfin[i]]
            self.last_live.append(([walk(i, steps - 1, int(bp_h[steps - 1, 2, i, n]))[0] for n in range(live_h[i])],
                                   scores_h[i][:live_h[i]]))
            extra = (([d[0] for d in done], dscores),) if return_all else ()
            if not done:
                results.append(([start_idx, end_idx], [], False) + extra)
                continue
            best = dscores.index(max(dscores))
            paths.append((i, len(results), done[best][1]))
            results.append((done[best][0], [], True) + extra)
        if return_alphas and paths:
            idx = torch.tensor([r for _, _, rows in paths for r in rows], dtype=torch.int64).to(dev)
            got = alphas.view(T * R, P).index_select(0, idx).cpu()
            syncs += 1
            o = 0
            for i, slot, rows in paths:
                al = torch.cat([torch.ones(1, P), got[o:o + len(rows)]], 0)
                o += len(rows)
                if encoder_out.dim() == 4:  # (steps+1, S, S) like the reference's seqs_alpha
                    al = al.view(-1, encoder_out.size(1), encoder_out.size(2))
                results[slot] = (results[slot][0], al.tolist(), True) + results[slot][3:]
        self.last_stats = {"steps": steps, "host_syncs": syncs}
        return results


class BaselineBatchedBeamSearch:
    """Beam search of the baseline (LSTM) captioner over B images per call (the reference has none: the
    semantics are ``attention_caption_image_beam_search``'s with the baseline recurrence). The state after
    feeding the image feature to the LSTM from a zero state is the initial (h, c) of all k beams of an image
    (that step's output, which predicts START in training, is discarded); sequences start as [START] with
    score 0; a step is h, c = LSTM(embedding(prev), (h, c)), logits = linear(h), then the selection and
    bookkeeping of ``BatchedBeamSearch`` on the same two device entry points. Rows i*k .. i*k+k-1 belong to
    image i. Per step: embed_gather, capmi_lstm_step_fwd, the R x V x H GEMM, capmi_beam_select,
    capmi_beam_advance; no host sync but the ``sync_every`` read of the count of images still live."""

    def __init__(self, decoder, beam_size):
        self.dec = decoder
        self.k = int(beam_size)
        if self.k < 1:
            raise ValueError("beam_size must be >= 1")
        if self.k > 16:
            raise ValueError("beam_size must be <= 16")
        self.last_stats = None
        self.last_live = None

    @torch.no_grad()
    def search(self, img_features, start_idx, end_idx, max_steps=50, return_all=False, sync_every=8):
        """img_features (B, M): the encoder's output. Returns a list of B tuples (sequence, [], finished) [+
        (finished sequences, their scores) with ``return_all``]; failure: ([start, end], [], False).
        ``last_stats`` = steps run and host syncs taken; ``last_live`` = per image (sequences, scores) of the
        beams still live at the stop."""
        from .baseline_eval import STEP_FUSED, lstm_step
        dec = self.dec
        if not img_features.is_cuda:
            raise RuntimeError("capmi baseline decoder path needs HIP tensors")
        dev = img_features.device
        feats = img_features.contiguous().float()
        B, k = feats.size(0), self.k
        R = B * k
        M, D = dec.embed_size, dec.hidden_size
        emb, w_lin, b_lin = dec.embedding.weight, dec.linear.weight, dec.linear.bias
        V = w_lin.shape[0]
        if feats.dim() != 2 or feats.size(1) != M:
            raise ValueError(f"img_features must be (B, {M})")
        T = int(max_steps) + 1
        sync_every = max(1, int(sync_every))
        f = dict(device=dev, dtype=torch.float32)
        scratch = None if STEP_FUSED else torch.empty(4, R, 4 * D, **f)
        h0, c0 = torch.empty(B, D, **f), torch.empty(B, D, **f)
        lstm_step(dec, B, h0, c0, x=feats, ld_x=M, scratch=scratch)
        h = h0.repeat_interleave(k, 0).contiguous()
        c = c0.repeat_interleave(k, 0).contiguous()
        xin = torch.empty(R, M, **f)
        h2, c2 = torch.empty(R, D, **f), torch.empty(R, D, **f)
        logits = torch.empty(R, V, **f)
        cand_v = torch.empty(R * k, **f)
        cand_w = torch.empty(R * k, dtype=torch.int32, device=dev)
        prev = torch.full((R,), start_idx, dtype=torch.int64, device=dev)
        # every small piece of beam state in one int32 buffer: one copy brings it to the host
        sizes = dict(bp=T * 3 * R, fin_count=B, fin_step=R, fin_slot=R, fin_score=R, live=B, scores=R,
                     images_live=1, parent=R, word=R, top=R)
        state = torch.zeros(sum(sizes.values()), dtype=torch.int32, device=dev)
        off, o = {}, 0
        for name, n in sizes.items():
            off[name] = (o, o + n)
            o += n

        def piece(buf, name, as_float=False):
            v = buf[off[name][0]:off[name][1]]
            return v.view(torch.float32) if as_float else v

        bp = piece(state, "bp").view(T, 3, R)
        live, images_live = piece(state, "live"), piece(state, "images_live")
        live.fill_(k)
        images_live.fill_(B)
        scores, top = piece(state, "scores", True), piece(state, "top", True)
        parent, word = piece(state, "parent"), piece(state, "word")
        fin_count, fin_step, fin_slot = piece(state, "fin_count"), piece(state, "fin_step"), piece(state, "fin_slot")
        fin_score = piece(state, "fin_score", True)

        steps = syncs = 0
        for t_ in range(T):
            K.embed_gather(emb, prev, R, 1, 1, xin, M)
            lstm_step(dec, R, h2, c2, x=xin, ld_x=M, h_prev=h, c_prev=c, scratch=scratch)
            K.gemm(K.problem(R, V, D, h2, D, w_lin, D, logits, V, bias=b_lin), AK, BW, K.TILE_64)
            K.beam_select(logits, scores, live, t_ == 0, B, k, V, cand_v, cand_w, parent, word, top)
            K.beam_advance(parent, word, top, live, B, k, D, end_idx, t_, h2, c2, h, c, prev, scores,
                           bp[t_, 0], bp[t_, 1], bp[t_, 2], fin_count, fin_step, fin_slot, fin_score, images_live)
            steps += 1
            if steps % sync_every == 0 and steps < T:
                syncs += 1
                if int(images_live.item()) == 0:
                    break
        host = state.cpu()
        syncs += 1
        bp_h = piece(host, "bp").view(T, 3, B, k).numpy()
        live_h, nfin = piece(host, "live").tolist(), piece(host, "fin_count").tolist()
        fstep, fslot = piece(host, "fin_step").view(B, k).tolist(), piece(host, "fin_slot").view(B, k).tolist()
        fscore = piece(host, "fin_score", True).view(B, k).tolist()
        scores_h = piece(host, "scores", True).view(B, k).tolist()

        def walk(i, t_, slot):
            """the words of the beam selected at step t_ as slot, back through the back-pointers"""
            words = []
            while True:
                row = int(bp_h[t_, 0, i, slot])
                words.append(int(bp_h[t_, 1, i, slot]))
                if t_ == 0:
                    break
                t_ -= 1
                slot = int(bp_h[t_, 2, i, row])
            return [start_idx] + words[::-1]

        results, self.last_live = [], []
        for i in range(B):
            done = [walk(i, fstep[i][q], fslot[i][q]) for q in range(nfin[i])]
            dscores = fscore[i][:nfin[i]]
            self.last_live.append(([walk(i, steps - 1, int(bp_h[steps - 1, 2, i, n])) for n in range(live_h[i])],
                                   scores_h[i][:live_h[i]]))
            extra = ((done, dscores),) if return_all else ()
            if not done:
                results.append(([start_idx, end_idx], [], False) + extra)
                continue
            results.append((done[dscores.index(max(dscores))], [], True) + extra)
        self.last_stats = {"steps": steps, "host_syncs": syncs}
        return results
