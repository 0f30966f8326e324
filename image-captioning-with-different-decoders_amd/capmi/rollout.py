"""The free-running (inference) decode step of each decoder, defined once: what batched beam search
(capmi.beam) and the sampled rollouts (capmi.sample) run per step.

A stepper is built from (decoder, features, rows_per_image): R = B * rows_per_image rows, rows i*n .. i*n+n-1
belonging to image i. Its constructor does the per-batch work and allocates every per-step buffer; ``step``
issues one decode step's launches for all R rows, reading the state ``h`` / ``c`` and leaving the new one in
``h2`` / ``c2``. Beam search gathers h2 / c2 into h / c through capmi_beam_advance; the samplers, whose rows
carry their own state on, ``swap`` the two pairs.
"""
import torch

from . import baseline_core as core
from . import baseline_eval
from . import kernels as K
from ._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_NMAJOR_W as BW


def attention_params(d):
    return dict(W_ea=d.attention.enc_att.weight, b_ea=d.attention.enc_att.bias,
                W_da=d.attention.dec_att.weight, b_da=d.attention.dec_att.bias,
                wf=d.attention.full_att.weight.view(-1), bf=d.attention.full_att.bias,
                W_ih=d.decode_step.weight_ih, W_hh=d.decode_step.weight_hh,
                b_ih=d.decode_step.bias_ih, b_hh=d.decode_step.bias_hh,
                W_h=d.h_lin.weight, b_h=d.h_lin.bias, W_c=d.c_lin.weight, b_c=d.c_lin.bias,
                W_fb=d.f_beta.weight, b_fb=d.f_beta.bias, W_fc=d.fc.weight, b_fc=d.fc.bias,
                emb=d.embedding.weight)


class _Stepper:
    def swap(self):
        self.h, self.h2, self.c, self.c2 = self.h2, self.h, self.c2, self.c


class AttentionStepper(_Stepper):
    """The soft-attention decoder's step: embed_gather, the grouped h-GEMM (att_dec | f_beta | W_hh h),
    capmi_beam_att_fwd (score, softmax, context, gate: features and ``enc_att`` features once per image, nothing
    expanded per row), the input GEMM, capmi_lstm_cell_fwd and the vocabulary GEMM. Per batch: ``enc_att`` of
    the features and the initial state from their mean, once per image."""

    def __init__(self, decoder, features, rows_per_image):
        """features: (B, S, S, E) or (B, P, E)."""
        p = self.p = attention_params(decoder)
        dev = self.dev = features.device
        B, E = features.size(0), features.size(-1)
        enc = self.enc = features.reshape(B, -1, E).contiguous().float()
        P, n = enc.size(1), rows_per_image
        R = B * n
        A, D = p["W_ea"].shape[0], p["W_hh"].shape[1]
        M, V = p["emb"].shape[1], p["W_fc"].shape[0]
        X = M + E
        self.B, self.n, self.R, self.P, self.V, self.D = B, n, R, P, V, D
        self.dims = (A, E, M, X)
        f = dict(device=dev, dtype=torch.float32)
        self.att_enc = torch.empty(B * P, A, **f)
        K.gemm(K.problem(B * P, A, E, enc, E, p["W_ea"], E, self.att_enc, A, bias=p["b_ea"]), AK, BW, K.TILE_64)
        mean = torch.empty(B, E, **f)
        K.mean_rows(enc, B, P, E, mean)
        h0, c0 = torch.empty(B, D, **f), torch.empty(B, D, **f)
        K.gemm([K.problem(B, D, E, mean, E, p["W_h"], E, h0, D, bias=p["b_h"]),
                K.problem(B, D, E, mean, E, p["W_c"], E, c0, D, bias=p["b_c"])], AK, BW, K.TILE_64)
        self.h = h0.repeat_interleave(n, 0).contiguous()
        self.c = c0.repeat_interleave(n, 0).contiguous()
        self.xin = torch.zeros(R, X, **f)
        self.p_ad, self.p_gate = torch.empty(R, A, **f), torch.empty(R, E, **f)
        self.p_hh, self.p_x = torch.empty(R, 4 * D, **f), torch.empty(R, 4 * D, **f)
        self.e_ws = torch.empty(R, P, **f)
        self.act, self.h2, self.c2 = torch.empty(R, 4 * D, **f), torch.empty(R, D, **f), torch.empty(R, D, **f)

    def step(self, prev, logits_out, live, alpha_out=None):
        """prev (R,) int64: the token every row feeds; logits_out (R, V). live (B,) int32: the rows of each
        image capmi_beam_att_fwd serves; alpha_out (R, P): the step's attention weights, when wanted."""
        p, R, P, V, D = self.p, self.R, self.P, self.V, self.D
        A, E, M, X = self.dims
        h, xin, p_ad, p_gate, p_hh = self.h, self.xin, self.p_ad, self.p_gate, self.p_hh
        K.embed_gather(p["emb"], prev, R, 1, 1, xin, X)
        K.gemm([K.problem(R, A, D, h, D, p["W_da"], D, p_ad, A),
                K.problem(R, E, D, h, D, p["W_fb"], D, p_gate, E),
                K.problem(R, 4 * D, D, h, D, p["W_hh"], D, p_hh, 4 * D)], AK, BW, K.TILE_64)
        K.beam_att_fwd(self.enc, self.att_enc, p_ad, 1, 0, p["b_da"], p["wf"], p["bf"], p_gate, 1, 0, p["b_fb"], live,
                       self.B, self.n, P, A, E, self.e_ws, alpha_out=alpha_out, x_out=xin[:, M:], ld_x=X)
        K.gemm(K.problem(R, 4 * D, X, xin, X, p["W_ih"], X, self.p_x, 4 * D, bias=p["b_ih"], bias2=p["b_hh"]),
               AK, BW, K.TILE_64)
        K.lstm_cell_fwd(self.p_x, 1, 0, None, p_hh, 1, 0, self.c, R, D, self.h2, self.c2, self.act)
        K.gemm(K.problem(R, V, D, self.h2, D, p["W_fc"], D, logits_out, V, bias=p["b_fc"]), AK, BW, K.TILE_64)


class BaselineStepper(_Stepper):
    """The baseline (LSTM) decoder's step: embed_gather, one ``baseline_core.step`` from the embedding
    (capmi_lstm_step_fwd, or its sequence when ``baseline_eval.STEP_FUSED`` is off at construction) and the
    R x V x H GEMM. Per batch: the state after feeding the image feature to the LSTM from a zero state is the
    initial (h, c) of all rows of an image (that step's output, which predicts START in training, is
    discarded)."""

    def __init__(self, decoder, features, rows_per_image):
        """features (B, M): the encoder's output."""
        core.check_inputs(features)
        dev = self.dev = features.device
        feats = features.contiguous().float()
        B, n = feats.size(0), rows_per_image
        R = B * n
        M, D = decoder.embed_size, decoder.hidden_size
        p = self.p = core.params(decoder)
        V = p[5].shape[0]
        if feats.dim() != 2 or feats.size(1) != M:
            raise ValueError(f"img_features must be (B, {M})")
        self.B, self.n, self.R, self.V, self.D, self.M = B, n, R, V, D, M
        f = dict(device=dev, dtype=torch.float32)
        self.fused = baseline_eval.STEP_FUSED
        self.scratch = None if self.fused else torch.empty(4, R, 4 * D, **f)
        h0, c0 = torch.empty(B, D, **f), torch.empty(B, D, **f)
        core.step(p, B, M, D, h0, c0, x=feats, ld_x=M, scratch=self.scratch, fused=self.fused)
        self.h = h0.repeat_interleave(n, 0).contiguous()
        self.c = c0.repeat_interleave(n, 0).contiguous()
        self.xin = torch.empty(R, M, **f)
        self.h2, self.c2 = torch.empty(R, D, **f), torch.empty(R, D, **f)

    def step(self, prev, logits_out):
        """prev (R,) int64: the token every row feeds; logits_out (R, V)."""
        p, R, V, D, M = self.p, self.R, self.V, self.D, self.M
        K.embed_gather(p[0], prev, R, 1, 1, self.xin, M)
        core.step(p, R, M, D, self.h2, self.c2, x=self.xin, ld_x=M, h_prev=self.h, c_prev=self.c,
                  scratch=self.scratch, fused=self.fused)
        K.gemm(K.problem(R, V, D, self.h2, D, p[5], D, logits_out, V, bias=p[6]), AK, BW, K.TILE_64)
