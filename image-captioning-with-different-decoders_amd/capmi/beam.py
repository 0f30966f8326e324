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
rows of one batch of B*k, the features stay once per image (the step is capmi.rollout.AttentionStepper's),
and selection and bookkeeping are HIP kernels (csrc/beam.hip, driven by ``_BeamState``), so a decode step is
a fixed launch sequence without a host sync.

``BaselineBatchedBeamSearch`` is the same search for the baseline (LSTM) captioner: the step is
capmi.rollout.BaselineStepper's (one capmi_lstm_step_fwd launch, csrc/baseline_step.hip), the beam state,
selection and bookkeeping are the same.
"""
import torch

from . import kernels as K
from ._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_NMAJOR_W as BW
from .rollout import AttentionStepper, BaselineStepper, attention_params


class BeamSearch:
    def __init__(self, decoder, beam_size):
        self.dec = decoder
        self.k = int(beam_size)
        if self.k < 1:
            raise ValueError("beam_size must be >= 1")

    @torch.no_grad()
    def search(self, encoder_out, start_idx, end_idx, max_steps=50, return_all=False):
        """encoder_out: (1, 14, 14, E) or (1, P, E) features of ONE image. Returns
        (sequence list[int], alphas list (steps, P), finished bool) like the reference
        (failure: ([start, end], [], False)); with ``return_all`` also (every finished sequence,
        their scores)."""
        if self.dec.use_bert:
            raise NotImplementedError("beam search with BERT features (the reference notes it fails too)")
        p = attention_params(self.dec)
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


class _BeamState:
    """What a batched search keeps beside its stepper ``st`` (R = B * k rows): the logits of a step, the
    candidates, the token every row feeds next, and every small piece of beam state in one int32 buffer, so
    that one copy brings it to the host."""

    def __init__(self, st, start_idx, end_idx, max_steps, sync_every):
        self.st, self.start_idx, self.end_idx = st, start_idx, end_idx
        B, k, R, dev = st.B, st.n, st.R, st.dev
        self.T = T = int(max_steps) + 1
        self.sync_every = max(1, int(sync_every))
        self.logits = torch.empty(R, st.V, device=dev, dtype=torch.float32)
        self.cand_v = torch.empty(R * k, device=dev, dtype=torch.float32)
        self.cand_w = torch.empty(R * k, dtype=torch.int32, device=dev)
        self.prev = torch.full((R,), start_idx, dtype=torch.int64, device=dev)
        sizes = dict(bp=T * 3 * R, fin_count=B, fin_step=R, fin_slot=R, fin_score=R, live=B, scores=R,
                     images_live=1, parent=R, word=R, top=R)
        self.state = torch.zeros(sum(sizes.values()), dtype=torch.int32, device=dev)
        self.off, o = {}, 0
        for name, n in sizes.items():
            self.off[name] = (o, o + n)
            o += n
        dev_piece = lambda name, as_float=False: self.piece(self.state, name, as_float)  # noqa: E731
        self.bp = dev_piece("bp").view(T, 3, R)
        self.live, self.images_live = dev_piece("live"), dev_piece("images_live")
        self.live.fill_(k)
        self.images_live.fill_(B)
        self.select = (dev_piece("parent"), dev_piece("word"), dev_piece("top", True))
        self.scores = dev_piece("scores", True)
        self.fin = (dev_piece("fin_count"), dev_piece("fin_step"), dev_piece("fin_slot"), dev_piece("fin_score", True))
        self.steps = self.syncs = 0

    def piece(self, buf, name, as_float=False):
        v = buf[self.off[name][0]:self.off[name][1]]
        return v.view(torch.float32) if as_float else v

    def advance(self, t_):
        """Selection and bookkeeping of step t_ on ``logits``: the stepper's h2 / c2 are gathered into its h / c
        and ``prev`` is set. True when the ``sync_every`` read finds no image with a live beam."""
        st, bp = self.st, self.bp[t_]
        B, k = st.B, st.n
        K.beam_select(self.logits, self.scores, self.live, t_ == 0, B, k, st.V, self.cand_v, self.cand_w, *self.select)
        K.beam_advance(*self.select, self.live, B, k, st.D, self.end_idx, t_, st.h2, st.c2, st.h, st.c, self.prev,
                       self.scores, bp[0], bp[1], bp[2], *self.fin, self.images_live)
        self.steps += 1
        if self.steps % self.sync_every == 0 and self.steps < self.T:
            self.syncs += 1
            return int(self.images_live.item()) == 0
        return False

    def finish(self, return_all):
        """One copy to the host, then the sequences rebuilt from the back-pointers. Returns (results, last_live,
        paths): per image (sequence, [], finished) [+ (finished sequences, their scores)]; per image (sequences,
        scores) of the beams still live; per finished image (image, slot in results, the rows of the (T * R, P)
        alphas its best sequence took)."""
        B, k, R, T, steps = self.st.B, self.st.n, self.st.R, self.T, self.steps
        start_idx, end_idx = self.start_idx, self.end_idx
        host = self.state.cpu()
        self.syncs += 1
        bp_h = self.piece(host, "bp").view(T, 3, B, k).numpy()
        live_h, nfin = self.piece(host, "live").tolist(), self.piece(host, "fin_count").tolist()
        fstep, fslot = self.piece(host, "fin_step").view(B, k).tolist(), self.piece(host, "fin_slot").view(B, k).tolist()
        fscore = self.piece(host, "fin_score", True).view(B, k).tolist()
        scores_h = self.piece(host, "scores", True).view(B, k).tolist()

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

        results, paths, last_live = [], [], []
        for i in range(B):
            done = [walk(i, fstep[i][q], fslot[i][q]) for q in range(nfin[i])]
            dscores = fscore[i][:nfin[i]]
            last_live.append(([walk(i, steps - 1, int(bp_h[steps - 1, 2, i, n]))[0] for n in range(live_h[i])],
                              scores_h[i][:live_h[i]]))
            extra = (([d[0] for d in done], dscores),) if return_all else ()
            if not done:
                results.append(([start_idx, end_idx], [], False) + extra)
                continue
            best = dscores.index(max(dscores))
            paths.append((i, len(results), done[best][1]))
            results.append((done[best][0], [], True) + extra)
        return results, last_live, paths

    def finish_device(self, emit_end=False, drop=(), fallback_live=False, length_alpha=0.0):
        """The back-trace as one launch (``capmi_beam_backtrack``), with no copy of the state to the host: per
        image the best finished beam (score / (step + 1) ** length_alpha; the raw score at 0, as ``finish``), or
        with ``fallback_live`` the best live beam of an image without one, as a column of the sampler's token
        table. ``drop``: at most two token ids left out; the final END stays only with ``emit_end``. Returns device
        tensors: tokens (T, B) int32 (-1 past a column's words), lens / finished (B,) int32, score (B,) fp32 (the
        raw beam score), steps () int32."""
        drop_a, drop_b = tuple(int(w) for w in drop) + (-1,) * (2 - len(drop))  # (a search checks its arguments first)
        B, k, T, dev = self.st.B, self.st.n, self.T, self.st.dev
        ints = torch.empty(T + 2, B, dtype=torch.int32, device=dev)
        out = dict(tokens=ints[:T], lens=ints[T], finished=ints[T + 1],
                   score=torch.empty(B, dtype=torch.float32, device=dev),
                   steps=torch.full((), self.steps, dtype=torch.int32, device=dev))
        K.beam_backtrack(self.bp, *self.fin, self.live, self.scores, self.steps, B, k, T, self.end_idx, out["tokens"],
                         out["lens"], out["finished"], out["score"], drop_a=drop_a, drop_b=drop_b, emit_end=emit_end,
                         fallback_live=fallback_live, length_alpha=length_alpha)
        return out


class BatchedBeamSearch(BeamSearch):
    """Beam search over B images per call. The beams of image i are rows i*k .. i*k+k-1 of every per-step
    tensor, its live ones compacted to the front. The decode step is ``rollout.AttentionStepper``'s (features
    and ``enc_att`` features once per image). Selection and bookkeeping are two device entry points
    (``capmi_beam_select``, ``capmi_beam_advance``), so a step needs no host sync: the host reads the device
    count of images that still have live beams every ``sync_every`` steps only, and rebuilds the sequences after
    the loop from the back-pointers. ``search_device`` leaves that walk on the device too (``capmi_beam_backtrack``)
    and returns the captions as a token table."""

    def __init__(self, decoder, beam_size):
        super().__init__(decoder, beam_size)
        if self.k > 16:
            raise ValueError("beam_size must be <= 16")
        self.last_stats = None
        self.last_live = None

    def _run(self, st, start_idx, end_idx, max_steps, return_all, sync_every, step_args=lambda bs, t_: ()):
        """The search on stepper ``st``; ``step_args(bs, t_)``: what its ``step`` takes at step t_ beside the
        tokens and the logits. Returns ``_BeamState.finish``'s results and paths."""
        bs = self._loop(st, start_idx, end_idx, max_steps, sync_every, step_args)
        results, self.last_live, paths = bs.finish(return_all)
        self.last_stats = {"steps": bs.steps, "host_syncs": bs.syncs}
        return results, paths

    @staticmethod
    def _loop(st, start_idx, end_idx, max_steps, sync_every, step_args):
        """The decode steps of a search: the ``_BeamState`` they leave."""
        bs = _BeamState(st, start_idx, end_idx, max_steps, sync_every)
        for t_ in range(bs.T):
            st.step(bs.prev, bs.logits, *step_args(bs, t_))
            if bs.advance(t_):
                break
        return bs

    def _run_device(self, st, start_idx, end_idx, max_steps, sync_every, finish_args, step_args=lambda bs, t_: ()):
        """``_run`` with the back-trace on the device: ``_BeamState.finish_device``'s tensors."""
        if not float(finish_args["length_alpha"]) >= 0.0:
            raise ValueError("length_alpha must be >= 0")
        finish_args["drop"] = tuple(finish_args["drop"])
        if len(finish_args["drop"]) > 2:
            raise ValueError("search_device drops at most two token ids")
        bs = self._loop(st, start_idx, end_idx, max_steps, sync_every, step_args)
        out = bs.finish_device(**finish_args)
        self.last_live = None  # the live beams stay on the device
        self.last_stats = {"steps": bs.steps, "host_syncs": bs.syncs}
        return out

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
        st = AttentionStepper(self.dec, encoder_out, self.k)
        T, R, P = int(max_steps) + 1, st.R, st.P
        alphas = torch.zeros(T, R, P, device=st.dev, dtype=torch.float32) if return_alphas else None
        results, paths = self._run(st, start_idx, end_idx, max_steps, return_all, sync_every,
                                   lambda bs, t_: (bs.live, alphas[t_] if return_alphas else None))
        if return_alphas and paths:
            idx = torch.tensor([r for _, _, rows in paths for r in rows], dtype=torch.int64).to(st.dev)
            got = alphas.view(T * R, P).index_select(0, idx).cpu()
            self.last_stats["host_syncs"] += 1
            o = 0
            for i, slot, rows in paths:
                al = torch.cat([torch.ones(1, P), got[o:o + len(rows)]], 0)
                o += len(rows)
                if encoder_out.dim() == 4:  # (steps+1, S, S) like the reference's seqs_alpha
                    al = al.view(-1, encoder_out.size(1), encoder_out.size(2))
                results[slot] = (results[slot][0], al.tolist(), True) + results[slot][3:]
        return results

    @torch.no_grad()
    def search_device(self, encoder_out, start_idx, end_idx, max_steps=50, sync_every=8, emit_end=False, drop=(),
                      fallback_live=False, length_alpha=0.0):
        """The launches of ``search`` without alphas, then ``_BeamState.finish_device`` (its arguments and
        return): the captions stay on the device, as a (max_steps + 1, B) token table a ``DeviceCaptionScorer``
        reads. ``last_stats`` counts the ``sync_every`` reads only; ``last_live`` is None."""
        if self.dec.use_bert:
            raise NotImplementedError("beam search with BERT features (the reference notes it fails too)")
        st = AttentionStepper(self.dec, encoder_out, self.k)
        return self._run_device(st, start_idx, end_idx, max_steps, sync_every,
                                dict(emit_end=emit_end, drop=drop, fallback_live=fallback_live,
                                     length_alpha=length_alpha), lambda bs, t_: (bs.live, None))


class BaselineBatchedBeamSearch(BatchedBeamSearch):
    """Beam search of the baseline (LSTM) captioner over B images per call (the reference has none: the
    semantics are ``attention_caption_image_beam_search``'s with the baseline recurrence). Sequences start as
    [START] with score 0; the decode step is ``rollout.BaselineStepper``'s (h, c = LSTM(embedding(prev), (h, c)),
    logits = linear(h), from the state the image feature leaves), the selection, bookkeeping and stop test are
    ``BatchedBeamSearch``'s. Rows i*k .. i*k+k-1 belong to image i."""

    @torch.no_grad()
    def search(self, img_features, start_idx, end_idx, max_steps=50, return_all=False, sync_every=8):
        """img_features (B, M): the encoder's output. Returns a list of B tuples (sequence, [], finished) [+
        (finished sequences, their scores) with ``return_all``]; failure: ([start, end], [], False).
        ``last_stats`` = steps run and host syncs taken; ``last_live`` = per image (sequences, scores) of the
        beams still live at the stop."""
        st = BaselineStepper(self.dec, img_features, self.k)
        return self._run(st, start_idx, end_idx, max_steps, return_all, sync_every)[0]

    @torch.no_grad()
    def search_device(self, img_features, start_idx, end_idx, max_steps=50, sync_every=8, emit_end=False, drop=(),
                      fallback_live=False, length_alpha=0.0):
        """``BatchedBeamSearch.search_device`` on the baseline step."""
        if getattr(self.dec, "use_bert", False):
            raise NotImplementedError("beam search with BERT features (the reference notes it fails too)")
        st = BaselineStepper(self.dec, img_features, self.k)
        return self._run_device(st, start_idx, end_idx, max_steps, sync_every,
                                dict(emit_end=emit_end, drop=drop, fallback_live=fallback_live,
                                     length_alpha=length_alpha))
