"""Self-critical sequence training (SCST) of both captioners on the capmi kernels.

The model samples ``n`` captions per image (capmi.sample), every caption is scored with CIDEr-D against the image's
references on the device (``capmi_cider_reward`` on the sampler's own token table, no host copy), the reward minus
a baseline (the mean of the image's other samples, or the greedy rollout's reward) weights the caption's
log-probabilities, and one teacher-forced pass over the sampled captions gives the policy gradient
(``capmi_pg_ce_fwd_bwd`` into ``baseline_core.backward``, or into capmi.decoder_group for the attention captioner,
whose image features stay once per image through forward and backward).

``CiderRefs``          the device tables ``capmi_cider_reward`` reads, built once from the training captions
``cider_rewards_host`` the same per-hypothesis reward in fp64 Python, from the definitions (CPU fallback, oracle)
``reward_mix``         of both steps: train on a weighted sum of CIDEr-D, BLEU-4 and ROUGE-L instead (the tables and
                       kernels of capmi.devscore, csrc/score.hip)
``BaselineSelfCriticalStep`` / ``AttentionSelfCriticalStep``  rollout, reward, advantage, forward, weighted loss,
                       backward, clamp + Adam

The reference project has no self-critical training; its CIDEr scorer (eval_func/cider/cider_scorer.py) defines the
reward, scored for one hypothesis at a time with the document frequencies of the whole reference corpus.
"""
import math
import types

import numpy as np
import torch

from . import baseline_core as core
from . import kernels as K
from ._lib import CAPMI_SCST_GREEDY, CAPMI_SCST_MEAN
from .baseline_train import BaselineTrainStep
from .decoder_core import PNAMES
from .decoder_fn import decoder_params, gemm_flags
from .sample import BaselineBatchedSampler, BatchedSampler
from .scoring import CIDER_N, CIDER_SIGMA, _ngrams

MAX_REF_WORDS = 63   # a reference and its END fill the 64 words a hypothesis may have
MAX_TOKEN = 65533    # token + 1 in a 16-bit field of the n-gram key, 0 kept for 'no word'
MAX_HYP_WORDS = 64


def _flat_keys(tokens, rid):
    """n-gram keys of the concatenated references ``tokens`` (uint64 token + 1) with reference ids ``rid``: per
    order the key of every window that stays inside one reference, and the reference it belongs to."""
    keys, owner = [], []
    N = tokens.shape[0]
    for order in range(1, CIDER_N + 1):
        m = N - order + 1
        if m <= 0:
            break
        ok = rid[:m] == rid[order - 1:]
        k = np.zeros(m, dtype=np.uint64)
        for j in range(order):
            k |= tokens[j:j + m] << np.uint64(48 - 16 * j)
        keys.append(k[ok])
        owner.append(rid[:m][ok])
    if not keys:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    return np.concatenate(keys), np.concatenate(owner)


def key_order(keys):
    """The n-gram order (1..4) a key carries: its non-zero 16-bit fields."""
    keys = np.asarray(keys, dtype=np.uint64)
    m = np.uint64(0xffff)
    return (1 + ((keys >> np.uint64(32)) & m != 0).astype(np.int64) + ((keys >> np.uint64(16)) & m != 0)
            + (keys & m != 0))


class CiderRefs:
    """The reference corpus of the CIDEr-D reward, as tables on ``device`` (layouts: capmi_cider_reward in
    capmi.h). Host copies of every table stay in ``host`` (numpy); ``df`` and ``idf64`` are the corpus's document
    frequencies and the idf before its rounding to fp32, by sorted key."""

    @classmethod
    def build(cls, references_by_image, end_idx=None, device="cpu"):
        """references_by_image: per image key 0, 1, .. the list of its reference captions (token-id lists, START /
        END / PAD stripped). ``end_idx``: END is appended to every reference (score hypotheses with
        ``score_end=True`` to match)."""
        self = cls()
        refs, img_of_ref, img_count, by_image = [], [], [], []
        for image, caps in enumerate(references_by_image):
            caps = [list(int(w) for w in c) for c in caps]
            if not caps:
                raise ValueError(f"image {image} has no reference caption")
            for c in caps:
                if len(c) > MAX_REF_WORDS:
                    raise ValueError(f"a reference of image {image} has {len(c)} words (at most {MAX_REF_WORDS})")
                if c and (min(c) < 0 or max(c) > MAX_TOKEN):
                    raise ValueError(f"a reference of image {image} holds a token outside 0..{MAX_TOKEN}")
                refs.append(c + [int(end_idx)] if end_idx is not None else c)
                img_of_ref.append(image)
            img_count.append(len(caps))
            by_image.append(refs[len(refs) - len(caps):])
        if not refs:
            raise ValueError("CiderRefs needs at least one image")
        if end_idx is not None and not 0 <= int(end_idx) <= MAX_TOKEN:
            raise ValueError(f"end_idx outside 0..{MAX_TOKEN}")
        self.end_idx = None if end_idx is None else int(end_idx)
        self.references = by_image  # as scored: END appended
        n_images, n_refs = len(img_count), len(refs)
        lens = np.array([len(c) for c in refs], dtype=np.int64)
        tokens = np.array([w for c in refs for w in c], dtype=np.uint64) + np.uint64(1)
        rid = np.repeat(np.arange(n_refs, dtype=np.int64), lens)
        keys, owner = _flat_keys(tokens, rid)
        # a reference's distinct keys with their counts, references in order and keys ascending inside each
        order = np.lexsort((keys, owner))
        keys, owner = keys[order], owner[order]
        new = np.ones(keys.shape[0], dtype=bool)
        new[1:] = (keys[1:] != keys[:-1]) | (owner[1:] != owner[:-1])
        starts = np.flatnonzero(new)
        tf = np.diff(np.append(starts, keys.shape[0]))
        ekeys, eowner = keys[starts], owner[starts]
        # document frequency: the number of images whose reference set holds the key
        eimg = np.asarray(img_of_ref, dtype=np.int64)[eowner]
        o2 = np.lexsort((eimg, ekeys))
        k2, i2 = ekeys[o2], eimg[o2]
        new2 = np.ones(k2.shape[0], dtype=bool)
        new2[1:] = (k2[1:] != k2[:-1]) | (i2[1:] != i2[:-1])
        idf_keys, df = np.unique(k2[new2], return_counts=True)
        log_images = math.log(float(n_images)) if n_images != 1 else 1.0  # the scorers' quirk
        idf64 = log_images - np.log(np.maximum(1.0, df.astype(np.float64)))
        idf = idf64.astype(np.float32)
        # w_r = tf * idf as the kernel forms the hypothesis's: one fp32 product of the rounded idf
        ew = tf.astype(np.float32) * idf[np.searchsorted(idf_keys, ekeys)]
        norm2 = np.bincount(eowner * 4 + key_order(ekeys) - 1, weights=ew.astype(np.float64) ** 2,
                            minlength=4 * n_refs)
        if max(ekeys.shape[0], n_refs, n_images) >= 2 ** 31 - 1:
            raise ValueError("the reference tables are indexed with int32")
        self.n_images, self.n_refs, self.n_keys, self.log_images = n_images, n_refs, int(idf_keys.shape[0]), log_images
        self.df, self.idf64 = df, idf64
        self.host = dict(
            idf_keys=idf_keys, idf_vals=idf, ref_keys=ekeys, ref_w=ew,
            ref_off=np.concatenate(([0], np.cumsum(np.bincount(eowner, minlength=n_refs)))).astype(np.int32),
            ref_norm=np.sqrt(norm2).astype(np.float32).reshape(n_refs, 4),
            ref_bigrams=np.maximum(lens - 1, 0).astype(np.int32),
            img_off=np.concatenate(([0], np.cumsum(img_count))).astype(np.int32))
        self._counts = None
        return self.to(device)

    def to(self, device):
        self.device = torch.device(device)
        for name, a in self.host.items():
            if a.dtype == np.uint64:  # torch has no uint64 arithmetic: the bits travel as int64
                a = a.view(np.int64)
            setattr(self, name, torch.from_numpy(np.ascontiguousarray(a)).to(self.device))
        return self

    @property
    def nbytes(self):
        """Bytes of device memory the tables take."""
        return int(sum(a.nbytes for a in self.host.values()))

    def counts(self):
        """(per image the n-gram counts of every listed reference, the corpus's document frequencies), keyed by
        token tuples: what ``cider_rewards_host`` scores against. Built on first use."""
        if self._counts is None:
            per_image = [[_ngrams(r, CIDER_N) for r in caps] for caps in self.references]
            df = {}
            for counts in per_image:
                for g in set(g for c in counts for g in c):
                    df[g] = df.get(g, 0) + 1
            self._counts = (per_image, df)
        return self._counts


def cider_rewards_host(refs, hyps, image_keys, score_end=True, end_idx=None):
    """The reward of ``capmi_cider_reward`` in fp64 Python, from the definitions (capmi.scoring.cider's, for one
    hypothesis at a time against the corpus in ``refs``). hyps: token-id lists as a rollout emits them (a final
    ``end_idx`` included); ``score_end`` False drops that END. Returns a list of floats."""
    per_image, df = refs.counts()
    end_idx = refs.end_idx if end_idx is None else end_idx
    log_images, n, two_sigma2 = refs.log_images, CIDER_N, 2 * CIDER_SIGMA ** 2

    def tfidf(counts):
        vec, norm, bigrams = [{} for _ in range(n)], [0.0] * n, 0
        for g, tf in counts.items():
            k = len(g) - 1
            w = float(tf) * (log_images - math.log(max(1.0, float(df.get(g, 0)))))
            vec[k][g] = w
            norm[k] += w * w
            if k == 1:
                bigrams += tf
        return vec, [math.sqrt(x) for x in norm], bigrams

    ref_vecs = {}
    out = []
    for hyp, image in zip(hyps, image_keys):
        image = int(image)
        hyp = [int(w) for w in hyp]
        if len(hyp) > MAX_HYP_WORDS:
            raise ValueError(f"a hypothesis holds at most {MAX_HYP_WORDS} words")
        if not score_end and hyp and end_idx is not None and hyp[-1] == end_idx:
            hyp = hyp[:-1]
        if image not in ref_vecs:
            ref_vecs[image] = [tfidf(c) for c in per_image[image]]
        hv, hn, hl = tfidf(_ngrams(hyp, n))
        total = [0.0] * n
        for rv, rn, rl in ref_vecs[image]:
            penalty = math.exp(-(float(hl - rl) ** 2) / two_sigma2)
            for k in range(n):
                val = 0.0
                for g, w in hv[k].items():
                    wr = rv[k].get(g, 0.0)
                    val += min(w, wr) * wr
                if hn[k] != 0 and rn[k] != 0:
                    val /= hn[k] * rn[k]
                total[k] += val * penalty
        out.append(math.fsum(total) / n / len(ref_vecs[image]) * 10.0)
    return out


def hyps_from_table(tokens, lens):
    """The hypotheses of a (T, R) token table and its ``lens``, as lists on the host."""
    tok = tokens.t().tolist()
    return [row[:int(k)] for row, k in zip(tok, lens.tolist())]


class _SelfCriticalStep(BaselineTrainStep):
    """What the self-critical steps of both captioners share: the rollouts, pack / reward / advantage, the launch
    modes and ``last``. A subclass supplies its samplers (``_sampler``), the features of a batch (``_features``),
    the decoder's buffers (``_decoder_buffers``) and the teacher-forced pass with the weighted loss and the
    backward (``_policy_gradient``).

    ``refs``: the ``CiderRefs`` of the training captions, on the decoder's device. ``baseline``: "mean" (the mean
    reward of the image's other samples, ``num_samples`` >= 2) or "greedy" (the reward of one temperature-0 rollout
    per image).

    ``reward_mix``: None (CIDEr-D alone) or weights such as ``dict(cider=1.0, bleu4=0.5, rouge_l=0.0)``: the reward
    is their weighted sum of CIDEr-D, sentence-level BLEU-4 and ROUGE-L (``capmi_caption_stats``,
    ``capmi_reward_mix``; the greedy rollout's likewise), ``refs`` must then be a ``capmi.devscore.ScoreRefs`` and
    ``last`` also keeps ``cider``, ``bleu4`` and ``rouge_l`` per sampled row.

    ``graph=True`` captures everything after the rollouts (pack, reward, advantage, forward, weighted loss,
    backward, update) once per (B, n) into one linear HIP graph: the packed captions are always (B n, max_steps +
    2). The rollouts stay eager: they stop early on a host read.

    The returned loss and the tensors in ``last`` are the step's own buffers, overwritten by the next call of the
    same batch size: clone them to keep them. ``counts``: a capturing call counts as "capture", not as "replay".
    """

    def __init__(self, encoder, decoder, optimizer, refs, V, ctx=None, num_samples=5, temperature=1.0, top_k=0,
                 baseline="mean", max_steps=20, score_end=True, graph=False, start_idx=1, end_idx=2, pad_idx=0,
                 reward_mix=None):
        if baseline not in ("mean", "greedy"):
            raise ValueError('baseline must be "mean" or "greedy"')
        super().__init__(encoder, decoder, optimizer, ctx=ctx, graph=graph, ignore_index=pad_idx)
        self.n, self.baseline, self.max_steps = int(num_samples), baseline, int(max_steps)
        if baseline == "mean" and self.n < 2:
            raise ValueError('baseline "mean" needs num_samples >= 2 (the mean of the other samples)')
        if not 1 <= self.max_steps + 1 <= MAX_HYP_WORDS:
            raise ValueError(f"max_steps must be 0..{MAX_HYP_WORDS - 1} (a hypothesis of at most {MAX_HYP_WORDS} words)")
        self.refs, self.score_end = refs, bool(score_end)
        self.reward_mix = self._check_mix(reward_mix, refs)
        self._cider_refs = refs if self.reward_mix is None else refs.cider
        self.start_idx, self.end_idx, self.pad_idx = int(start_idx), int(end_idx), int(pad_idx)
        self.V = int(V)
        if self.V > MAX_TOKEN + 1:
            raise ValueError(f"the vocabulary must not exceed {MAX_TOKEN + 1} words (16-bit n-gram fields)")
        self.sampler = self._sampler(self.n, temperature, top_k)
        self.greedy_sampler = self._sampler(1, 0.0, 0) if baseline == "greedy" else None
        self.sync_every = 8
        self.last = None
        self._sc = {}

    @staticmethod
    def _check_mix(reward_mix, refs):
        """The weights (cider, bleu4, rouge_l) of a mixed reward, or None."""
        if reward_mix is None:
            return None
        from .devscore import METRICS, ScoreRefs
        if not isinstance(reward_mix, dict) or not reward_mix or set(reward_mix) - set(METRICS):
            raise ValueError(f"reward_mix must be a dict of weights over {METRICS}")
        weights = tuple(float(reward_mix.get(k, 0.0)) for k in METRICS)
        if not all(math.isfinite(w) for w in weights):
            raise ValueError("reward_mix weights must be finite")
        if not isinstance(refs, ScoreRefs):
            raise ValueError("reward_mix needs refs to be a capmi.devscore.ScoreRefs (BLEU and ROUGE-L tables)")
        return weights

    # ------------------------------------------------------------------ buffers
    def _sc_buffers(self, B, feats):
        sc = self._sc.get(B)
        if sc is not None:
            if sc.feats.shape != feats.shape:
                raise ValueError(f"the features of a batch of {B} were {tuple(sc.feats.shape)}, now "
                                 f"{tuple(feats.shape)}: one feature shape per batch size")
            return sc
        n, T = self.n, self.max_steps + 1
        R, dev = B * n, feats.device
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)  # noqa: E731
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
        sc = types.SimpleNamespace(
            feats=torch.zeros_like(feats), img_key=i32(B), tokens=i32(T, R), lens=i32(R),
            caps=torch.zeros(R, T + 1, dtype=torch.int64, device=dev), reward=f32(R), adv=f32(R), stats=f32(2),
            gtokens=i32(T, B), glens=i32(B), greward=f32(B),
            gcaps=torch.zeros(B, T + 1, dtype=torch.int64, device=dev), ginv=f32(1))
        if self.reward_mix is not None:  # the three components of the sampled and the greedy rows
            from ._lib import CAPMI_SCORE_STATS
            for name, rows in (("", R), ("g", B)):
                setattr(sc, name + "cider", f32(rows))
                setattr(sc, name + "bleu", f32(rows, 4))
                setattr(sc, name + "rouge", f32(rows))
                setattr(sc, name + "score_stats", i32(rows, CAPMI_SCORE_STATS))
        sc.ws, logp_cols = self._decoder_buffers(sc, B, R, T)
        sc.logp_rows = f32(R * logp_cols)
        self._sc[B] = sc
        return sc

    # ------------------------------------------------------------------ the step
    def _grad_half(self, sc, B, own_reward, own_greedy, with_update):
        """Everything after the rollouts, on the static buffers of ``sc``: a linear chain of launches."""
        n, T, ws = self.n, self.max_steps + 1, sc.ws
        R = B * n
        K.rollout_pack(sc.tokens, T, R, self.start_idx, self.end_idx, self.pad_idx, sc.lens, sc.caps, ws.count, ws.inv)
        if own_reward:
            self._reward(sc, sc.tokens, T, R, n, sc.lens, "", sc.reward)
        greedy = self.baseline == "greedy"
        if greedy and own_greedy:
            K.rollout_pack(sc.gtokens, T, B, self.start_idx, self.end_idx, self.pad_idx, sc.glens, sc.gcaps, None,
                           sc.ginv)
            self._reward(sc, sc.gtokens, T, B, 1, sc.glens, "g", sc.greward)
        K.scst_advantage(sc.reward, sc.greward if greedy else None, B, n,
                         CAPMI_SCST_GREEDY if greedy else CAPMI_SCST_MEAN, sc.adv, sc.stats)
        self._policy_gradient(sc, B)
        if with_update:
            self._step_all()
        return ws.loss

    def _reward(self, sc, tokens, T, R, n, lens, which, reward):
        """CIDEr-D into ``reward``; with a ``reward_mix`` the three metrics into the ``which`` ("" sampled, "g"
        greedy) component buffers and their weighted sum into ``reward``."""
        if self.reward_mix is None:
            K.cider_reward(tokens, T, R, n, lens, sc.img_key, self._cider_refs, self.V, self.end_idx, self.score_end,
                           reward)
            return
        cider, bleu, rouge = (getattr(sc, which + k) for k in ("cider", "bleu", "rouge"))
        K.cider_reward(tokens, T, R, n, lens, sc.img_key, self._cider_refs, self.V, self.end_idx, self.score_end, cider)
        K.caption_stats(tokens, T, R, n, lens, sc.img_key, self.refs, self.V, self.end_idx, self.score_end,
                        getattr(sc, which + "score_stats"), bleu, rouge)
        K.reward_mix(cider, bleu, rouge, R, *self.reward_mix, reward)

    def __call__(self, imgs, img_keys, seed=None, uniforms=None, rewards=None, greedy_rewards=None, update=True):
        """imgs: what the encoder takes, B images; img_keys (B,): their keys in ``refs``. ``seed`` / ``uniforms``:
        the sampler's. ``rewards`` (B n,) / ``greedy_rewards`` (B,) replace the reward kernel's output (tests, other
        metrics). Returns the loss -sum adv logp / count (device tensor (1,), no host sync); ``last`` keeps
        reward_mean, greedy_reward_mean, lens, tokens, logp (the sampler's), adv, rewards, greedy_rewards, caps
        (the packed captions) and logp_rows (the teacher-forced log-probabilities, a row per caption: R, max_steps
        + 2 for the baseline captioner, whose step 0 is the image; R, max_steps + 1 for the attention captioner)
        as device tensors. ``update=False`` (eager): gradients only, left in the optimizer's flat buffer."""
        if not imgs.is_cuda:
            raise RuntimeError(f"{type(self).__name__} needs HIP tensors")
        with torch.no_grad():
            feats = self._features(imgs)
        B = feats.size(0)
        sc = self._sc_buffers(B, feats)
        sc.feats.copy_(feats)
        keys = torch.as_tensor(img_keys)
        if keys.numel() != B:
            raise ValueError("one image key per image")
        sc.img_key.copy_(keys.reshape(-1), non_blocking=True)
        tokens, logp, _, _ = self.sampler.sample_device(sc.feats, self.start_idx, self.end_idx, self.max_steps,
                                                        seed=seed, uniforms=uniforms, sync_every=self.sync_every)
        sc.tokens.copy_(tokens)
        greedy = self.greedy_sampler is not None
        if rewards is not None:
            sc.reward.copy_(rewards.reshape(-1))
        if greedy:
            if greedy_rewards is not None:
                sc.greward.copy_(greedy_rewards.reshape(-1))
            else:
                sc.gtokens.copy_(self.greedy_sampler.sample_device(sc.feats, self.start_idx, self.end_idx,
                                                                   self.max_steps, sync_every=self.sync_every)[0])
        own = (rewards is None, greedy_rewards is None)
        dp = self.ctx.distributed
        if self.graph_mode and update:
            loss = self._replay_half(sc, B, own)
        else:
            self.counts["eager"] += 1
            loss = self._grad_half(sc, B, *own, with_update=update and not dp)
        if update and dp:
            self._finish_dp()
        self.last = dict(reward_mean=sc.stats[0:1], greedy_reward_mean=sc.stats[1:2] if greedy else None,
                         lens=sc.lens, tokens=sc.tokens, logp=logp, adv=sc.adv, rewards=sc.reward,
                         greedy_rewards=sc.greward if greedy else None, caps=sc.caps,
                         logp_rows=sc.logp_rows.view(B * self.n, -1))
        if self.reward_mix is not None:  # the components of the kernels' own rewards (stale under ``rewards=``)
            self.last.update(cider=sc.cider, bleu4=sc.bleu[:, 3], rouge_l=sc.rouge)
        return loss

    # ------------------------------------------------------------------ graph
    def _replay_half(self, sc, B, own):
        key = (B,) + own
        g = self._gcache.get(key)
        if g is None:
            if len(self._gcache) >= self.graph_cache_size:
                self.counts["eager"] += 1
                return self._grad_half(sc, B, *own, with_update=not self.ctx.distributed)
            # one pass on a side stream, update held back: every lazily made workspace exists before the capture
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._grad_half(sc, B, *own, with_update=False)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode=self.capture_error_mode):
                self._grad_half(sc, B, *own, with_update=not self.ctx.distributed)
            self._gcache[key] = g
            self.counts["capture"] += 1
        else:
            self.counts["replay"] += 1
        g.replay()
        return sc.ws.loss


class BaselineSelfCriticalStep(_SelfCriticalStep):
    """One self-critical step of the baseline (LSTM) captioner (module docstring, ``_SelfCriticalStep``)."""

    def __init__(self, encoder, decoder, optimizer, refs, ctx=None, num_samples=5, temperature=1.0, top_k=0,
                 baseline="mean", max_steps=20, score_end=True, graph=False, start_idx=1, end_idx=2, pad_idx=0,
                 encoder_optimizer=None, reward_mix=None):
        if encoder_optimizer is not None:
            raise NotImplementedError("self-critical training with a trainable embed Linear: the features are "
                                      "computed once, without a graph")
        super().__init__(encoder, decoder, optimizer, refs, decoder.linear.weight.shape[0], ctx, num_samples,
                         temperature, top_k, baseline, max_steps, score_end, graph, start_idx, end_idx, pad_idx,
                         reward_mix)

    def _sampler(self, n, temperature, top_k):
        return BaselineBatchedSampler(self.decoder, n, temperature, top_k)

    def _features(self, imgs):
        return self.encoder(imgs).float()

    def _decoder_buffers(self, sc, B, R, T):
        return self._buffers(R, T + 1), T + 1

    def _policy_gradient(self, sc, B):
        n, ws = self.n, sc.ws
        R, L = B * n, self.max_steps + 2
        # rows b n .. b n + n - 1 carry image b's feature, as in the sampler
        ws.X[0].view(B, n, -1).copy_(sc.feats.unsqueeze(1).expand(B, n, sc.feats.size(1)))
        core.forward(self.decoder, sc.caps, ws.X, ws.GX, ws.H, ws.C, ws.logits, ws.ACT, fused=self.fused_fwd,
                     scratch=(None, ws.HH, ws.zeros, None))
        # step 0 scores the image feature against START, which is no action: t_first = 1, target caps[t]
        K.pg_ce_fwd_bwd(ws.logits, sc.caps, R, L, L, self.V, 0, sc.lens, 1, sc.adv, ws.inv, sc.logp_rows,
                        ws.loss_rows, ws.dlogits, True)
        K.loss_finalize_dev(ws.loss_rows, R * L, ws.inv, ws.loss)
        self._backward(sc.caps, ws, None)


class AttentionSelfCriticalStep(_SelfCriticalStep):
    """One self-critical step of the soft-attention captioner (``_SelfCriticalStep``). The features (B, P, E),
    whatever P the encoder gives, are computed once per image under ``no_grad`` and are never repeated per sample:
    the rollouts run on ``capmi_beam_att_fwd`` (capmi.sample.BatchedSampler) and the teacher-forced pass over the
    R = B n sampled captions on capmi.decoder_group (``capmi_att_group_bwd`` / ``capmi_att_group_enc_grad``
    backward). Steps: features, rollouts (plus one greedy rollout per image for ``baseline="greedy"``), pack /
    reward / advantage, grouped forward, ``capmi_pg_ce_fwd_bwd`` (target caps[t + 1], live steps 0 .. lens - 1,
    time-major dlogits), ``capmi_loss_finalize_dev``, grouped backward, clamp + Adam.

    The loss is -sum adv logp / count. There is no doubly-stochastic term (``alpha_c`` does not apply to sampled
    captions with padded steps) and no dropout: the teacher-forced log-probabilities are the sampler's. The GEMMs
    follow the decoder's ``compute_precision``. Not taken: a data-parallel context, a trainable encoder, BERT /
    dense embeddings."""

    def __init__(self, encoder, decoder, optimizer, refs, ctx=None, num_samples=5, temperature=1.0, top_k=0,
                 baseline="mean", max_steps=20, score_end=True, graph=False, start_idx=1, end_idx=2, pad_idx=0,
                 reward_mix=None):
        from .decoder_group import N_MAX
        if getattr(decoder, "use_bert", False):
            raise NotImplementedError("self-critical training with BERT / dense word embeddings: the sampler has "
                                      "no features for the tokens it draws")
        if any(q.requires_grad for q in encoder.parameters()):
            raise NotImplementedError("self-critical training with a trainable encoder: the features are computed "
                                      "once per step, without a graph")
        if ctx is not None and ctx.distributed:
            raise NotImplementedError("data-parallel self-critical training of the attention captioner")
        if int(num_samples) > N_MAX:
            raise ValueError(f"num_samples must be <= {N_MAX} (the rows of an image one workgroup serves)")
        super().__init__(encoder, decoder, optimizer, refs, decoder.fc.weight.shape[0], ctx, num_samples, temperature,
                         top_k, baseline, max_steps, score_end, graph, start_idx, end_idx, pad_idx, reward_mix)
        named = dict(decoder.named_parameters())
        self.need = [k for k in PNAMES if named[k].requires_grad]
        self._named = named

    def _sampler(self, n, temperature, top_k):
        return BatchedSampler(self.decoder, n, temperature, top_k)

    def _features(self, imgs):
        f = self.encoder(imgs).float()
        return f.reshape(f.size(0), -1, f.size(-1)).contiguous()

    def _decoder_buffers(self, sc, B, R, T):
        from .decoder_group import GroupedDecoder
        dev = sc.feats.device
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        sc.core = GroupedDecoder()  # one per batch size: a captured graph keeps its workspace
        ws = types.SimpleNamespace(count=torch.zeros(1, dtype=torch.int32, device=dev), inv=f32(1), loss=f32(1),
                                   loss_rows=f32(R * T), dlogits=f32(T * R, self.V))
        return ws, T

    def _policy_gradient(self, sc, B):
        n, T, ws = self.n, self.max_steps + 1, sc.ws
        R, L = B * n, T + 1
        p = decoder_params(self.decoder)
        preds, _, st = sc.core.forward(p, sc.feats, sc.caps, n, gemm_flags=gemm_flags(self.decoder))
        # every step is an action: t_first = 0, target caps[t + 1]
        K.pg_ce_fwd_bwd(preds, sc.caps, R, T, L, self.V, 1, sc.lens, 0, sc.adv, ws.inv, sc.logp_rows, ws.loss_rows,
                        ws.dlogits, True)
        K.loss_finalize_dev(ws.loss_rows, R * T, ws.inv, ws.loss)
        grads = {k: self._named[k].grad for k in self.need}
        if "attention.full_att.weight" in grads:
            grads["attention.full_att.weight"] = grads["attention.full_att.weight"].view(-1)
        sc.core.backward(p, st, grads, ws.dlogits, need=self.need)
