"""Sampled caption rollouts on the capmi kernels: the third decode mode beside teacher-forced evaluation
(capmi.evalpass, capmi.baseline_eval) and beam search (capmi.beam).

``BatchedSampler`` draws ``num_samples`` captions per image from the attention decoder's own distribution
(temperature and top-k sampling, or the greedy rollout at temperature 0) and records the log-probability of
every token it emits. The recurrence is ``BatchedBeamSearch``'s, on the same kernels; the sampling stage is one
launch per step (``capmi_sample_step``, csrc/sample.hip) and all randomness is one table of uniforms drawn
before the loop, so every draw can be reproduced: sample j of image i at step t uses ``uniforms[t, i*n + j]``
and nothing else. ``BaselineBatchedSampler`` is the same for the baseline (LSTM) captioner.

The reference project has no sampler; the semantics of a draw are stated at ``capmi_sample_step`` in capmi.h.
"""
import torch

from . import kernels as K
from .baseline_core import check_inputs
from .rollout import AttentionStepper, BaselineStepper

KEEP_LOGITS_MAX_BYTES = 256 << 20


def _check_args(num_samples, temperature, top_k):
    n, temp, top_k = int(num_samples), float(temperature), int(top_k)
    if n < 1:
        raise ValueError("num_samples must be >= 1")
    if not temp >= 0:
        raise ValueError("temperature must be >= 0 (0: greedy)")
    if top_k < 0:
        raise ValueError("top_k must be >= 0 (0: the whole vocabulary)")
    return n, temp, top_k


class _Rollout:
    """What both samplers share: the uniforms, the per-row state in one int32 buffer, the ``sample_step`` call,
    the ``sync_every`` stop test and the rebuild of the sequences on the host."""

    def _begin(self, dev, B, V, max_steps, seed, uniforms, keep_logits, sync_every):
        n = self.n
        self.R = R = B * n
        self.T = T = int(max_steps) + 1
        self.sync_every = max(1, int(sync_every))
        if uniforms is None:
            gen = torch.Generator(device=dev)
            if seed is None:
                gen.seed()
            else:
                gen.manual_seed(int(seed))
            uniforms = torch.rand(T, R, generator=gen, device=dev, dtype=torch.float32)
        else:
            if tuple(uniforms.shape) != (T, R):
                raise ValueError(f"uniforms must be (max_steps + 1, B * num_samples) = ({T}, {R})")
            uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        self.u = uniforms
        self.last_logits = None
        if keep_logits:
            if T * R * V * 4 > KEEP_LOGITS_MAX_BYTES:
                raise ValueError("keep_logits: the (T, R, V) logits would take more than 256 MB")
            self.last_logits = torch.zeros(T, R, V, device=dev, dtype=torch.float32)
        else:
            self._logits = torch.empty(R, V, device=dev, dtype=torch.float32)
        # tokens (T, R) | logp (T, R) as float bits | alive (R) | rows_live (1): one copy brings it to the host
        self.state = torch.zeros(2 * T * R + R + 1, dtype=torch.int32, device=dev)
        self.tokens = self.state[:T * R].view(T, R)
        self.logp = self.state[T * R:2 * T * R].view(torch.float32).view(T, R)
        self.alive = self.state[2 * T * R:2 * T * R + R]
        self.rows_live = self.state[2 * T * R + R:]
        self.tokens.fill_(-1)
        self.alive.fill_(1)
        self.rows_live.fill_(R)
        self.steps = self.syncs = 0

    def _logits_at(self, t_):
        return self._logits if self.last_logits is None else self.last_logits[t_]

    def _draw(self, logits, t_, V, end_idx, prev):
        """the step's sampling launch; True when the ``sync_every`` read finds every row finished"""
        K.sample_step(logits, self.R, V, self.u[t_], self.temperature, self.top_k, end_idx, t_, self.alive, prev,
                      self.tokens[t_], self.logp[t_], self.rows_live)
        self.steps += 1
        if self.steps % self.sync_every == 0 and self.steps < self.T:
            self.syncs += 1
            return int(self.rows_live.item()) == 0
        return False

    def _roll(self, st, start_idx, end_idx, step_args=lambda t_: ()):
        """The rollout on stepper ``st``; ``step_args(t_)``: what its ``step`` takes beside the tokens and the
        logits. Every row carries its own state on, so the stepper's two state pairs are swapped: nothing to
        gather."""
        prev = torch.full((st.R,), start_idx, dtype=torch.int64, device=st.dev)
        for t_ in range(self.T):
            logits = self._logits_at(t_)
            st.step(prev, logits, *step_args(t_))
            st.swap()
            if self._draw(logits, t_, st.V, end_idx, prev):
                break

    def _finish(self, B, start_idx, end_idx):
        """list of B lists of n dicts (without alphas), and per row the number of tokens it emitted"""
        T, R, n = self.T, self.R, self.n
        host = self.state.cpu()
        self.syncs += 1
        tok = host[:T * R].view(T, R).t().tolist()
        lp = host[T * R:2 * T * R].view(torch.float32).view(T, R).t().tolist()
        out, counts = [], []
        for i in range(B):
            per = []
            for j in range(n):
                r = i * n + j
                words, finished = [], False
                for t_ in range(self.steps):
                    words.append(tok[r][t_])
                    if tok[r][t_] == end_idx:
                        finished = True
                        break
                tl = lp[r][:len(words)]
                per.append({"seq": [start_idx] + words if finished else words, "token_logp": tl,
                            "logp": float(sum(tl)), "finished": finished, "alphas": []})
                counts.append(len(words))
            out.append(per)
        self.last_stats = {"steps": self.steps, "host_syncs": self.syncs}
        return out, counts


class BatchedSampler(_Rollout):
    """``num_samples`` sampled captions per image from the attention decoder, B images per call. Rows i*n ..
    i*n+n-1 of every per-step tensor belong to image i; features and ``enc_att`` features exist once per image
    (``capmi_beam_att_fwd`` with all n rows of every image live). Rows are not compacted: a row that has
    emitted END keeps running through the recurrence and ``capmi_sample_step`` ignores it. No host sync in the
    loop but the read of the count of unfinished rows every ``sync_every`` steps."""

    def __init__(self, decoder, num_samples=1, temperature=1.0, top_k=0):
        self.n, self.temperature, self.top_k = _check_args(num_samples, temperature, top_k)
        if self.n > 16:
            raise ValueError("num_samples must be <= 16 (the rows capmi_beam_att_fwd serves per image)")
        self.dec = decoder
        self.last_stats = None
        self.last_logits = None

    @torch.no_grad()
    def sample(self, encoder_out, start_idx, end_idx, max_steps=50, seed=None, uniforms=None, return_alphas=False,
               keep_logits=False, sync_every=8):
        """encoder_out: (B, S, S, E) or (B, P, E). ``uniforms``: (max_steps + 1, B * num_samples) fp32 in [0, 1)
        (default: torch.rand on the device from a generator seeded with ``seed``). Returns a list of B lists of
        num_samples dicts: ``seq`` ([start, ..., end] when finished, else the max_steps + 1 tokens drawn),
        ``token_logp`` (one per emitted token), ``logp`` (their sum), ``finished``, ``alphas`` ((emitted + 1, S,
        S) or (emitted + 1, P) nested lists, a row of ones first, like beam search's; [] without
        ``return_alphas``). ``keep_logits``: every step's (R, V) logits stay in ``last_logits`` (T, R, V) on
        the device. ``last_stats`` = steps run and host syncs taken."""
        B, n = encoder_out.size(0), self.n
        P, alphas = self._rollout(encoder_out, start_idx, end_idx, max_steps, seed, uniforms, keep_logits, sync_every,
                                  return_alphas)
        out, counts = self._finish(B, start_idx, end_idx)
        if return_alphas:
            al_h = alphas.cpu()
            self.last_stats["host_syncs"] += 1
            for r, cnt in enumerate(counts):
                al = torch.cat([torch.ones(1, P), al_h[:cnt, r]], 0)
                if encoder_out.dim() == 4:  # (emitted + 1, S, S) like beam search's
                    al = al.view(-1, encoder_out.size(1), encoder_out.size(2))
                out[r // n][r % n]["alphas"] = al.tolist()
        return out

    def _rollout(self, encoder_out, start_idx, end_idx, max_steps, seed, uniforms, keep_logits, sync_every,
                 return_alphas=False):
        """The launches of one call; returns (P, the (T, R, P) alphas when wanted)."""
        if self.dec.use_bert:
            raise NotImplementedError("sampling with BERT features (as beam search)")
        dev, B, n = encoder_out.device, encoder_out.size(0), self.n
        # the table's own checks come before the stepper's launches
        self._begin(dev, B, self.dec.fc.weight.shape[0], max_steps, seed, uniforms, keep_logits, sync_every)
        st = AttentionStepper(self.dec, encoder_out, n)
        alphas = torch.zeros(self.T, st.R, st.P, device=dev, dtype=torch.float32) if return_alphas else None
        live = torch.full((B,), n, dtype=torch.int32, device=dev)
        self._roll(st, start_idx, end_idx, lambda t_: (live, alphas[t_] if return_alphas else None))
        return st.P, alphas

    @torch.no_grad()
    def sample_device(self, encoder_out, start_idx, end_idx, max_steps=50, seed=None, uniforms=None,
                      keep_logits=False, sync_every=8):
        """``sample`` without the copy to the host (and without alphas): the same launches, then the device views
        ``tokens`` (T, R) int32 (-1 where a row had finished or the loop had stopped), ``logp`` (T, R), ``alive``
        (R,) and the number of steps run, as ``BaselineBatchedSampler.sample_device`` returns them."""
        self._rollout(encoder_out, start_idx, end_idx, max_steps, seed, uniforms, keep_logits, sync_every)
        self.last_stats = {"steps": self.steps, "host_syncs": self.syncs}
        return self.tokens, self.logp, self.alive, self.steps


class BaselineBatchedSampler(_Rollout):
    """The same rollouts for the baseline (LSTM) captioner, on the recurrence of ``BaselineBatchedBeamSearch``:
    the state after feeding the image feature to the LSTM from a zero state is the initial (h, c) of all n rows
    of an image, then per step embed_gather, capmi_lstm_step_fwd, the R x V x H GEMM and capmi_sample_step.
    It returns no alphas."""

    def __init__(self, decoder, num_samples=1, temperature=1.0, top_k=0):
        self.n, self.temperature, self.top_k = _check_args(num_samples, temperature, top_k)
        self.dec = decoder
        self.last_stats = None
        self.last_logits = None

    @torch.no_grad()
    def sample(self, img_features, start_idx, end_idx, max_steps=50, seed=None, uniforms=None, keep_logits=False,
               sync_every=8):
        """img_features (B, M): the encoder's output. Returns what ``BatchedSampler.sample`` returns, every
        ``alphas`` empty."""
        self.sample_device(img_features, start_idx, end_idx, max_steps, seed, uniforms, keep_logits, sync_every)
        return self._finish(img_features.size(0), start_idx, end_idx)[0]

    @torch.no_grad()
    def sample_device(self, img_features, start_idx, end_idx, max_steps=50, seed=None, uniforms=None,
                      keep_logits=False, sync_every=8):
        """``sample`` without the copy to the host: the same launches, then the device views ``tokens`` (T, R)
        int32 (-1 where a row had finished or the loop had stopped), ``logp`` (T, R), ``alive`` (R,) and the
        number of steps run (T = max_steps + 1, R = B * num_samples). The views belong to this call: the next
        one allocates its own."""
        check_inputs(img_features)
        B = img_features.size(0)
        # the table's own checks come before the stepper's launch
        self._begin(img_features.device, B, self.dec.linear.weight.shape[0], max_steps, seed, uniforms, keep_logits,
                    sync_every)
        self._roll(BaselineStepper(self.dec, img_features, self.n), start_idx, end_idx)
        self.last_stats = {"steps": self.steps, "host_syncs": self.syncs}
        return self.tokens, self.logp, self.alive, self.steps
