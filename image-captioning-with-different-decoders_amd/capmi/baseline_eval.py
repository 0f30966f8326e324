"""Batched teacher-forced validation of the baseline (LSTM) captioner (reference models/baseline.py:267-374,
built there for batch 1).

``BaselineTeacherForcedEval`` runs the decoder's no-grad forward over a batch of captions of any lengths in any
order and reduces the (B, T, V) logits on the device: per caption the loss the reference computes for that
caption alone (cross entropy averaged over its own n rows, step t scored against ``caption[t]``: step 0, fed
the image feature, against START), the greedy tokens and the top-1 / top-5 hit counts. The LSTM is causal and
its rows are independent, so nothing is sorted or reindexed: every row runs all T = L steps and the rows past a
caption's end are masked by the reductions. Nothing is read back inside the call.

Launches: embed_gather; one hoisted (T*B) x 4H x M GEMM (both LSTM biases in its epilogue) into ``pre``; T
launches of capmi_lstm_step_fwd (``STEP_FUSED``; the three-launch sequence of the training forward otherwise)
writing H[t] time-major; the hoisted vocabulary GEMM written batch-first; eval_rows_at(tgt_off=0);
eval_captions_ce.
"""
import torch

from . import kernels as K
from ._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_NMAJOR_W as BW
from .baseline_fn import _params

N_SCALARS = 3  # rows of the packed result: cap_loss (fp32 bits), top1, top5
STEP_FUSED = True  # capmi_lstm_step_fwd per step; False: capmi_gemm + capmi_lstm_cell_fwd


def check_inputs(img_features, captions):
    """What ``baseline_fn.baseline_forward`` asks of its inputs, with its messages."""
    if not (img_features.is_cuda and captions.is_cuda):
        raise RuntimeError("capmi baseline decoder path needs HIP tensors")
    if captions.dtype != torch.int64:
        raise TypeError("captions must be int64")


def lstm_step(dec, R, h_out, c_out, *, pre=None, x=None, ld_x=0, h_prev=None, c_prev=None, scratch=None,
              fused=None):
    """One inference step of ``dec.lstm`` over R rows: ``pre`` (R, 4H) already holds the input product and the
    biases, or ``x`` (R, M) is multiplied here. ``fused`` False takes the training forward's sequence (GEMMs
    into ``scratch`` (4, R, 4H): the two products, zeros for a missing c_prev and the cell kernel's activation
    output; then the cell kernel): kept selectable for measurements and tests."""
    _, w_ih, w_hh, b_ih, b_hh, _, _ = _params(dec)
    M, H = dec.embed_size, dec.hidden_size
    if STEP_FUSED if fused is None else fused:
        K.lstm_step_fwd(R, M, H, h_out, c_out, pre=pre, x=x, ld_x=ld_x, h_prev=h_prev, c_prev=c_prev,
                        w_ih=w_ih if x is not None else None, w_hh=w_hh if h_prev is not None else None,
                        b_ih=b_ih if pre is None else None, b_hh=b_hh if pre is None else None)
        return
    gx, hh = scratch[0], scratch[1]
    if x is not None:
        K.gemm(K.problem(R, 4 * H, M, x, ld_x or M, w_ih, M, gx, 4 * H, bias=b_ih, bias2=b_hh), AK, BW, K.TILE_64)
        pre = gx
    if h_prev is not None:
        K.gemm(K.problem(R, 4 * H, H, h_prev, H, w_hh, H, hh, 4 * H), AK, BW, K.TILE_64)
    if c_prev is None:
        c_prev = scratch[2].view(-1)[:R * H].zero_()
    K.lstm_cell_fwd(pre, 1, 0, None, hh if h_prev is not None else None, 1 if h_prev is not None else 0, 0, c_prev,
                    R, H, h_out, c_out, scratch[3])


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
        check_inputs(img_features, captions)
        emb_w, w_ih, w_hh, b_ih, b_hh, w_lin, b_lin = _params(dec)
        caps = captions.contiguous()
        B, L = caps.shape
        lengths = [int(n) for n in caption_lengths]
        if len(lengths) != B:
            raise ValueError(f"{len(lengths)} caption lengths for a batch of {B}")
        if min(lengths) < 2 or max(lengths) > L:
            raise ValueError(f"caption lengths must lie in [2, {L}] (START .. END)")
        T, M, H, V = L, dec.embed_size, dec.hidden_size, w_lin.shape[0]
        dev = img_features.device
        f = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        lens = torch.tensor(lengths, dtype=torch.int32).to(dev, non_blocking=True)
        ws = dec._capmi_ws(dev)
        X = torch.empty(T, B, M, **f)
        X[0].copy_(img_features.float())  # step 0 = the image feature (reference :104)
        if T > 1:  # steps 1.. = embedding(captions[:, :-1]) (reference :98-101)
            K.embed_gather(emb_w, caps, B, L, T - 1, X[1:], M)
        pre = torch.empty(T * B, 4 * H, **f)
        K.gemm_sk(K.problem(T * B, 4 * H, M, X, M, w_ih, M, pre, 4 * H, bias=b_ih, bias2=b_hh), AK, ws, K.TILE_AUTO)
        Hs = torch.empty(T, B, H, **f)
        C = torch.empty(2, B, H, **f)
        scratch = None if STEP_FUSED else torch.empty(4, B, 4 * H, **f)
        for t in range(T):
            lstm_step(dec, B, Hs[t], C[t & 1], pre=pre[t * B:], h_prev=Hs[t - 1] if t > 0 else None,
                      c_prev=C[(t - 1) & 1] if t > 0 else None, scratch=scratch)
        logits = torch.empty(B, T, V, **f)
        # row r = t*B + b of the (T*B, V) product lands at logits[b][t] (baseline_fn's remap)
        K.gemm_sk(K.problem(T * B, V, H, Hs, H, w_lin, H, logits, T * V, c_r1=B, c_s2=V, bias=b_lin), AK, ws,
                  K.TILE_AUTO)
        loss_rows = torch.empty(B * T, **f)
        rank = torch.empty(B * T, **i32)
        packed = torch.empty(N_SCALARS * B + B * T, **i32)
        out = unpack(packed, B, T)
        K.eval_rows_at(logits, caps, B, T, L, V, 0, lens, loss_rows, out["pred"], rank)
        K.eval_captions_ce(loss_rows, rank, lens, B, T, out["cap_loss"], out["top1"], out["top5"])
        out["lengths"] = lengths
        self.last_stats = {"launches": 2, "host_syncs": 0, "step_launches": T if STEP_FUSED else 2 * T - 1}
        return out


def unpack(packed, B, T):
    """Views of a packed result buffer (device or host): see ``BaselineTeacherForcedEval.__call__``."""
    sc, pred = packed[:N_SCALARS * B].view(N_SCALARS, B), packed[N_SCALARS * B:].view(B, T)
    return {"cap_loss": sc[0].view(torch.float32), "top1": sc[1], "top5": sc[2], "pred": pred, "packed": packed}
