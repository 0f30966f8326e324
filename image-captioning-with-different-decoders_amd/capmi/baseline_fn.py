"""The baseline decoder (reference models/baseline.py:24-111) as an autograd function on the capmi kernels: an
LSTM over [image feature, embedding(captions[:, :-1])] with teacher forcing, then Linear to the vocabulary.

SURVEY.md §8f rank 4. The forward and the backward through time are capmi.baseline_core's, on the unfused
step sequence (capmi_gemm + capmi_lstm_cell_fwd / capmi_lstm_cell_bwd) and fresh buffers per call; the
gradient of the logits arrives batch-first.
"""
import types

import torch

from . import baseline_core as core
from . import kernels as K


class BaselineDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dec, img_features, captions, *params):
        B, L = captions.shape
        T, M, Hd, V = L, dec.embed_size, dec.hidden_size, params[5].shape[0]
        e = lambda *shape: torch.empty(*shape, device=img_features.device, dtype=torch.float32)  # noqa: E731
        caps = captions.contiguous()
        X = e(T, B, M)
        X[0].copy_(img_features.float())  # step 0 = the image feature (reference :104)
        GX, H, C, ACT, out = e(T * B, 4 * Hd), e(T, B, Hd), e(T, B, Hd), e(T, B, 4 * Hd), e(B, T, V)
        core.forward(dec, caps, X, GX, H, C, out, ACT, fused=False,
                     scratch=(None, e(B, 4 * Hd), torch.zeros(B, Hd, device=img_features.device), None))
        ctx.dec = dec
        ctx.img_dtype = img_features.dtype
        ctx.save_for_backward(caps, X, H, C, ACT, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        caps, X, H, C, ACT, *params = ctx.saved_tensors
        T, B, M = X.shape
        Hd, V = H.shape[2], params[5].shape[0]
        e = lambda *shape: torch.empty(*shape, device=X.device, dtype=torch.float32)  # noqa: E731
        ws = types.SimpleNamespace(X=X, H=H, C=C, ACT=ACT, dH=e(T * B, Hd), DG=e(T, B, 4 * Hd), DHR=e(B, Hd),
                                   DC=[e(B, Hd), e(B, Hd)], DX=e(T, B, M), gb=e(4 * Hd),
                                   cs_v=e(K.colsum_work_size(B * T, V)), cs_g=e(K.colsum_work_size(T * B, 4 * Hd)),
                                   zeros=torch.zeros(B, Hd, device=X.device))
        # no embedding gradient at T == 1: no caption token is fed
        grads = {n: torch.empty_like(q) for n, q in zip(core.PNAMES, params)
                 if q.requires_grad and (T > 1 or n != "embedding.weight")}
        core.backward(ctx.dec, caps, ws, dout.float().contiguous(), grads, need_dx=True)
        g_img = ws.DX[0].to(ctx.img_dtype) if ctx.needs_input_grad[1] else None
        return (None, g_img, None) + tuple(grads.get(n) for n in core.PNAMES)


def baseline_forward(dec, img_features, captions):
    core.check_inputs(img_features, captions)
    return BaselineDecoderFn.apply(dec, img_features.contiguous(), captions, *core.params(dec))
