"""Batched teacher-forced validation (reference models/attention.py:454-567, built there for batch 1).

``TeacherForcedEval`` runs the decoder's no-grad forward over a batch of captions of any lengths in any
order and reduces the (B, T, V) logits on the device (csrc/eval.hip): per caption the loss the reference
computes for that caption alone (cross entropy averaged over the caption's own rows plus the
doubly-stochastic regulariser over its own steps), the greedy tokens and the top-1 / top-5 hit counts.
Nothing is read back inside the call.
"""
import torch

from . import decoder_fn as DF
from . import kernels as K

N_SCALARS = 5  # rows of the packed result: cap_loss, cap_ce, cap_reg (fp32 bits), top1, top5


class TeacherForcedEval:
    """``__call__(encoder_out, captions, caption_lengths)`` -> dict of device tensors in the caller's order.

    ``last_stats``: ``launches`` = reduction launches after the decoder forward, ``host_syncs`` = device
    synchronisations or read-backs taken inside the call (none), ``sorted`` = whether the batch had to be
    reordered for the forward."""

    def __init__(self, decoder, alpha_c=1.0):
        self.dec = decoder
        self.alpha_c = float(alpha_c)
        self.last_stats = None

    @torch.no_grad()
    def __call__(self, encoder_out, captions, caption_lengths):
        """encoder_out (B, S, S, E) or (B, P, E); captions (B, L) int64, START..END padded to the batch
        maximum L; caption_lengths: the B true lengths (host ints), in any order.

        Returns ``cap_loss`` / ``cap_ce`` / ``cap_reg`` (B,) fp32, ``pred`` (B, T) int32 (-1 past a caption's
        end), ``top1`` / ``top5`` (B,) int32, ``decode_lengths`` (host list) and ``packed``: the int32 buffer
        all of them are views of ([N_SCALARS * B] scalars row-major, then pred), for a single copy to the host."""
        dec = self.dec
        enc, caps = DF._prep_inputs(dec, encoder_out, captions)
        B, L = caps.shape
        lengths = [int(l) for l in caption_lengths]
        if len(lengths) != B:
            raise ValueError(f"{len(lengths)} caption lengths for a batch of {B}")
        if min(lengths) < 2 or max(lengths) > L:
            raise ValueError(f"caption lengths must lie in [2, {L}] (START .. END)")
        decode_lengths = [l - 1 for l in lengths]
        # DecoderCore.forward is prefix-ragged: step t serves the first bt[t] rows, so longest first
        order = sorted(range(B), key=lambda i: -decode_lengths[i])
        reorder = order != list(range(B))
        dev = enc.device
        dl_sorted = [decode_lengths[i] for i in order]
        lens = torch.tensor(dl_sorted, dtype=torch.int32).to(dev, non_blocking=True)
        if reorder:
            inv = [0] * B
            for j, i in enumerate(order):
                inv[i] = j
            idx = torch.tensor([order, inv], dtype=torch.int64).to(dev, non_blocking=True)
            enc, caps = enc.index_select(0, idx[0]), caps.index_select(0, idx[0])
        p = DF.decoder_params(dec)
        preds, alphas, st = DF.CORE.forward(p, enc, caps, dl_sorted, dropout_p=0.0, training=False,
                                            emb_dense=DF.dense_embeddings(dec, caps),
                                            gemm_flags=DF.gemm_flags(dec))
        dm = st["dm"]
        T, V, P = dm.T, dm.V, alphas.shape[2]
        i32 = dict(device=dev, dtype=torch.int32)
        loss_rows = torch.empty(B * T, device=dev, dtype=torch.float32)
        rank = torch.empty(B * T, **i32)
        work = torch.empty(N_SCALARS * B + B * T, **i32)  # results in the forward's (sorted) order
        sc, pred = work[:N_SCALARS * B].view(N_SCALARS, B), work[N_SCALARS * B:].view(B, T)
        K.eval_rows(preds, caps, B, T, L, V, lens, loss_rows, pred, rank)
        K.eval_captions(loss_rows, rank, alphas, lens, B, T, P, self.alpha_c, sc[1].view(torch.float32),
                        sc[2].view(torch.float32), sc[0].view(torch.float32), sc[3], sc[4])
        if reorder:
            packed = torch.empty_like(work)
            torch.index_select(sc, 1, idx[1], out=packed[:N_SCALARS * B].view(N_SCALARS, B))
            torch.index_select(pred, 0, idx[1], out=packed[N_SCALARS * B:].view(B, T))
        else:
            packed = work
        out = unpack(packed, B, T)
        out["decode_lengths"] = decode_lengths
        self.last_stats = {"launches": 2, "host_syncs": 0, "sorted": reorder}
        return out


def unpack(packed, B, T):
    """Views of a packed result buffer (device or host): see ``TeacherForcedEval.__call__``."""
    sc, pred = packed[:N_SCALARS * B].view(N_SCALARS, B), packed[N_SCALARS * B:].view(B, T)
    f = torch.float32
    return {"cap_loss": sc[0].view(f), "cap_ce": sc[1].view(f), "cap_reg": sc[2].view(f), "top1": sc[3],
            "top5": sc[4], "pred": pred, "packed": packed}
