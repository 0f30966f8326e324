"""Batched teacher-forced validation of the baseline (LSTM) captioner (reference models/baseline.py:267-374,
built there for batch 1).

``BaselineTeacherForcedEval`` runs the decoder's no-grad forward over a batch of captions of any lengths in any
order and reduces the (B, T, V) logits on the device: per caption the loss the reference computes for that
caption alone (cross entropy averaged over its own n rows, step t scored against ``caption[t]``: step 0, fed
the image feature, against START), the greedy tokens and the top-1 / top-5 hit counts. The LSTM is causal and
its rows are independent, so nothing is sorted or reindexed: every row runs all T = L steps and the rows past a
caption's end are masked by the reductions. Nothing is read back inside the call.

Launches: capmi.baseline_core.forward (embed_gather; one hoisted (T*B) x 4H x M GEMM, both LSTM biases in its
epilogue; T launches of capmi_lstm_step_fwd with ``STEP_FUSED``, the two-launch sequence of the training forward
otherwise, writing H[t] time-major; the hoisted vocabulary GEMM written batch-first); eval_rows_at(tgt_off=0);
eval_captions_ce.
"""
import torch

from . import baseline_core as core
from . import kernels as K

N_SCALARS = 3  # rows of the packed result: cap_loss (fp32 bits), top1, top5
STEP_FUSED = True  # capmi_lstm_step_fwd per step; False: capmi_gemm + capmi_lstm_cell_fwd


def lstm_step(dec, R, h_out, c_out, *, fused=None, **kw):
    """``baseline_core.step`` on ``dec``'s parameters; ``fused`` None: ``STEP_FUSED`` as it stands at the call.
    The unfused sequence is kept selectable for measurements and tests."""
    core.step(core.params(dec), R, dec.embed_size, dec.hidden_size, h_out, c_out,
              fused=STEP_FUSED if fused is None else fused, **kw)


class BaselineTeacherForcedEval:
    """``__call__(img_features, captions, caption_lengths)`` -> dict of device tensors in the caller's order.

    ``last_stats``: ``launches`` = reduction launches after the decoder forward, ``host_syncs`` = device
    synchronisations or read-backs taken inside the call (none), ``step_launches`` = recurrence launches."""

    def __init__(self, decoder):
        self.dec = decoder
        self.last_stats = None

    @torch.no_grad()
    def __call__(self, img_features, captions, caption_lengths):
        """img_features (B, M); captions (B, L) int64, START..END padded to the batch maximum L;
        caption_lengths: the B true lengths (host ints), in any order.

        Returns ``cap_loss`` (B,) fp32, ``pred`` (B, T) int32 (-1 past a caption's end), ``top1`` / ``top5``
        (B,) int32, ``lengths`` (host list) and ``packed``: the int32 buffer all of them are views of
        ([N_SCALARS * B] scalars row-major, then pred), for a single copy to the host."""
        dec = self.dec
        core.check_inputs(img_features, captions)
        caps = captions.contiguous()
        B, L = caps.shape
        lengths = [int(n) for n in caption_lengths]
        if len(lengths) != B:
            raise ValueError(f"{len(lengths)} caption lengths for a batch of {B}")
        if min(lengths) < 2 or max(lengths) > L:
            raise ValueError(f"caption lengths must lie in [2, {L}] (START .. END)")
        T, M, H, V = L, dec.embed_size, dec.hidden_size, dec.linear.weight.shape[0]
        dev = img_features.device
        f = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        lens = torch.tensor(lengths, dtype=torch.int32).to(dev, non_blocking=True)
        fused = STEP_FUSED
        X = torch.empty(T, B, M, **f)
        X[0].copy_(img_features.float())  # step 0 = the image feature (reference :104)
        logits = torch.empty(B, T, V, **f)
        scratch = None if fused else (None, torch.empty(B, 4 * H, **f), torch.zeros(B, H, **f),
                                      torch.empty(B, 4 * H, **f))
        core.forward(dec, caps, X, torch.empty(T * B, 4 * H, **f), torch.empty(T, B, H, **f),
                     torch.empty(T, B, H, **f), logits, fused=fused, scratch=scratch)
        loss_rows = torch.empty(B * T, **f)
        rank = torch.empty(B * T, **i32)
        packed = torch.empty(N_SCALARS * B + B * T, **i32)
        out = unpack(packed, B, T)
        K.eval_rows_at(logits, caps, B, T, L, V, 0, lens, loss_rows, out["pred"], rank)
        K.eval_captions_ce(loss_rows, rank, lens, B, T, out["cap_loss"], out["top1"], out["top5"])
        out["lengths"] = lengths
        self.last_stats = {"launches": 2, "host_syncs": 0, "step_launches": T if fused else 2 * T - 1}
        return out


def unpack(packed, B, T):
    """Views of a packed result buffer (device or host): see ``BaselineTeacherForcedEval.__call__``."""
    sc, pred = packed[:N_SCALARS * B].view(N_SCALARS, B), packed[N_SCALARS * B:].view(B, T)
    return {"cap_loss": sc[0].view(torch.float32), "top1": sc[1], "top5": sc[2], "pred": pred, "packed": packed}
