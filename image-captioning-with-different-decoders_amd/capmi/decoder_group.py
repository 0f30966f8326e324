"""Teacher-forced forward and backward-through-time of the soft-attention decoder over row groups that share one
image's features: the gradient half of self-critical training (capmi.scst.AttentionSelfCriticalStep).

R = B * n captions, rows i*n .. i*n+n-1 belonging to image i (the sampler's layout). ``enc`` (B, P, E) and its
``enc_att`` projection exist once per image, forward and backward: the forward attention is
``capmi_beam_att_fwd`` with all n rows of every image live, the backward ``capmi_att_group_bwd`` per step and
``capmi_att_group_enc_grad`` once (csrc/att_group.hip). Nothing is replicated n times.

The recurrence is ``DecoderCore``'s unfused path (capmi.decoder_core) with R rows and what the sampled captions
do not need left out: all rows run all T = L - 1 steps (no ``bt``; ``capmi_pg_ce_fwd_bwd`` zeroes the gradient of
the padded steps), no regulariser, no dropout, no ``dup``. Hoisted as there: ``enc_att`` over B*P rows, the
embedding half of ``W_ih`` and ``fc`` over T*R rows, every weight gradient as one GEMM over the stacked per-step
gradients, ``dW_enc_att`` over the B*P rows of ``datt_enc``. ``h0`` / ``c0`` are computed per image and repeated n
times; their gradients are summed over each group (``capmi_segment_sum_rows``, j ascending) before the ``h_lin`` /
``c_lin`` gradients.

Per step forward: the grouped h-GEMM (``att_dec`` with its bias, so that its output is ``AD[t]``; ``f_beta``;
``W_hh h``), ``capmi_beam_att_fwd``, the input GEMM over the context columns, ``capmi_lstm_cell_fwd``. Backward:
``capmi_lstm_cell_bwd``, the dx GEMM, ``capmi_att_group_bwd``, the three dh GEMMs.

Every buffer is allocated once per (B, n, T, ...), so a pass can be captured in a HIP graph; the returned
predictions and alphas are the workspace's own, overwritten by the next forward of the same shape.
"""
import torch

from . import kernels as K
from ._lib import CAPMI_A_KMAJOR as AK, CAPMI_A_MMAJOR as AMM, CAPMI_B_KROWS as BKR
from ._lib import CAPMI_B_NMAJOR_W as BW
from .decoder_core import DecoderCore, DecoderDims

N_MAX = 16  # the rows capmi_beam_att_fwd / capmi_att_group_bwd serve per image

_gemm_into = DecoderCore._gemm_into


class GroupWorkspace:
    def __init__(self, dm, B, n, device):
        R, T, P, A, D, M, V, E, X = dm.B, dm.T, dm.P, dm.A, dm.D, dm.M, dm.V, dm.E, dm.X
        f = dict(device=device, dtype=torch.float32)
        e = torch.empty
        self.X = e(T, R, X, **f)
        self.mean, self.H0, self.C0 = e(B, E, **f), e(B, D, **f), e(B, D, **f)
        self.H, self.C = e(T + 1, R, D, **f), e(T + 1, R, D, **f)
        self.ACT, self.XEMB = e(T, R, 4 * D, **f), e(T, R, 4 * D, **f)
        self.AD, self.AWE, self.GATE = e(T, R, A, **f), e(T, R, E, **f), e(T, R, E, **f)
        self.ALPHA = e(T, R, P, **f)
        self.ATT_ENC = e(B, P, A, **f)
        self.score = e(R, P, **f)
        self.live = torch.full((B,), n, dtype=torch.int32, device=device)
        self.seg = torch.arange(0, R + 1, n, dtype=torch.int32, device=device)
        self.P_gate, self.P_hh = e(R, E, **f), e(R, 4 * D, **f)
        self.P_x = e(dm.s_x, R, 4 * D, **f)
        self.preds = e(R, T, V, **f)
        # backward
        self.DHD, self.DG = e(T, R, D, **f), e(T, R, 4 * D, **f)
        self.DGP, self.DAD, self.DE = e(T, R, E, **f), e(T, R, A, **f), e(T, R, P, **f)
        self.DALPHA = e(R, P, **f)
        self.DC = e(2, R, D, **f)
        self.P_dx = e(dm.s_dx, R, E, **f)
        self.P_dh = e(sum(dm.s_dh), R, D, **f)
        self.DH0, self.DH0G, self.DC0G = e(R, D, **f), e(B, D, **f), e(B, D, **f)
        self.DATT = e(B, P, A, **f)
        nblk = K.att_enc_grad_blocks(B, P)
        self.WF_PART, self.BF_PART = e(nblk, A, **f), e(nblk, 1, **f)
        self.scratch = e(max(T * R * M, 4 * B * D * 8), **f)
        self.sk = K.gemm_workspace(device)
        self.work = e(max(K.colsum_work_size(T * R, V), K.colsum_work_size(B * P, A),
                          K.colsum_work_size(T * R, 4 * D), K.colsum_work_size(T * R, E), 64), **f)


class GroupedDecoder:
    """Stateless apart from the per-shape workspace cache (one live shape at a time)."""

    def __init__(self):
        self._ws = {}

    def workspace(self, dm, B, n, device):
        key = (dm.key(), n, str(device))
        ws = self._ws.get(key)
        if ws is None:
            self._ws.clear()
            ws = self._ws[key] = GroupWorkspace(dm, B, n, device)
        return ws

    # ------------------------------------------------------------------ forward
    def forward(self, p, enc, caps, n, gemm_flags=0):
        """p: name -> tensor (decoder_core.PNAMES, full_att.weight flat). enc (B, P, E) contiguous fp32, once per
        image; caps (B n, L) int64, row i*n + j the j-th caption of image i. Returns (predictions (R, T, V),
        alphas (T, R, P) time-major, state); T = L - 1."""
        gf = gemm_flags
        B, P, E = enc.shape
        R, L = caps.shape
        if not 1 <= n <= N_MAX or R != B * n:
            raise ValueError(f"captions ({R}) must be {B} images x n rows, 1 <= n <= {N_MAX}")
        if L < 2:
            raise ValueError("captions need a START and at least one step")
        T = L - 1
        A, D = p["attention.enc_att.weight"].shape[0], p["decode_step.weight_hh"].shape[1]
        M, V = p["embedding.weight"].shape[1], p["fc.weight"].shape[0]
        dm = DecoderDims(R, T, L, P, A, D, M, V, E, gemm_flags=gf)  # the split-K factors of R-row step GEMMs
        ws = self.workspace(dm, B, n, enc.device)
        X = dm.X
        W_ih = p["decode_step.weight_ih"]
        K.embed_gather(p["embedding.weight"], caps, R, L, T, ws.X, X)
        # init_hidden_state once per image, repeated over the group
        K.mean_rows(enc, B, P, E, ws.mean)
        sh = min(8, max(1, E // 256))
        slab = ws.scratch[:2 * sh * B * D]
        K.gemm([K.problem(B, D, E, ws.mean, E, p["h_lin.weight"], E, slab, D, ksplit=sh, c_split_stride=B * D),
                K.problem(B, D, E, ws.mean, E, p["c_lin.weight"], E, slab[sh * B * D:], D, ksplit=sh,
                          c_split_stride=B * D)], AK, BW, K.TILE_64, flags=gf)
        K.splitk_reduce(slab, sh, B * D, B, D, D, ws.H0, D, bias=p["h_lin.bias"])
        K.splitk_reduce(slab[sh * B * D:], sh, B * D, B, D, D, ws.C0, D, bias=p["c_lin.bias"])
        ws.H[0].view(B, n, D).copy_(ws.H0.unsqueeze(1).expand(B, n, D))
        ws.C[0].view(B, n, D).copy_(ws.C0.unsqueeze(1).expand(B, n, D))
        # hoisted enc_att (once per image) and the embedding half of the LSTM input GEMM
        _gemm_into(ws, ws.ATT_ENC, A, B * P, A, E, enc, E, p["attention.enc_att.weight"], E, AK, BW,
                   bias=p["attention.enc_att.bias"], gf=gf)
        _gemm_into(ws, ws.XEMB, 4 * D, T * R, 4 * D, M, ws.X, X, W_ih, X, AK, BW,
                   bias=p["decode_step.bias_ih"], bias2=p["decode_step.bias_hh"], gf=gf)
        W_ih_awe = W_ih[:, M:]
        wf = p["attention.full_att.weight"]
        for t in range(T):
            h = ws.H[t]
            K.gemm([K.problem(R, A, D, h, D, p["attention.dec_att.weight"], D, ws.AD[t], A,
                              bias=p["attention.dec_att.bias"]),
                    K.problem(R, E, D, h, D, p["f_beta.weight"], D, ws.P_gate, E),
                    K.problem(R, 4 * D, D, h, D, p["decode_step.weight_hh"], D, ws.P_hh, 4 * D)],
                   AK, BW, K.TILE_64, flags=gf)
            K.beam_att_fwd(enc, ws.ATT_ENC, ws.AD[t], 1, 0, None, wf, p["attention.full_att.bias"], ws.P_gate, 1, 0,
                           p["f_beta.bias"], ws.live, B, n, P, A, E, ws.score, alpha_out=ws.ALPHA[t],
                           awe_out=ws.AWE[t], gate_out=ws.GATE[t], x_out=ws.X[t, :, M:], ld_x=X)
            K.gemm(K.problem(R, 4 * D, E, ws.X[t, :, M:], X, W_ih_awe, X, ws.P_x, 4 * D, ksplit=dm.s_x,
                             c_split_stride=R * 4 * D), AK, BW, K.TILE_64, flags=gf)
            K.lstm_cell_fwd(ws.P_x, dm.s_x, R * 4 * D, ws.XEMB[t], ws.P_hh, 1, 0, ws.C[t], R, D, ws.H[t + 1],
                            ws.C[t + 1], ws.ACT[t])
        _gemm_into(ws, ws.preds, T * V, T * R, V, D, ws.H[1:], D, p["fc.weight"], D, AK, BW, bias=p["fc.bias"],
                   c_r1=R, c_s2=V, gf=gf)
        state = dict(dm=dm, ws=ws, enc=enc, caps=caps, B=B, n=n, gflags=gf)
        return ws.preds, ws.ALPHA, state

    # ------------------------------------------------------------------ backward
    def backward(self, p, st, grads, dpred, need=None):
        """Writes parameter gradients into ``grads`` (name -> tensor, pre-allocated). dpred: the gradient of the
        predictions, time-major (T*R, V), row t*R + r (what capmi_pg_ce_fwd_bwd writes)."""
        dm, ws, enc, B, n, gf = st["dm"], st["ws"], st["enc"], st["B"], st["n"], st["gflags"]
        R, T, L, P, A, D, M, V, E, X = dm.B, dm.T, dm.L, dm.P, dm.A, dm.D, dm.M, dm.V, dm.E, dm.X
        need = set(grads) if need is None else set(need)
        W_ih = p["decode_step.weight_ih"]
        TR = T * R
        # ---- fc
        _gemm_into(ws, ws.DHD, D, TR, D, V, dpred, V, p["fc.weight"], D, AK, BKR, gf=gf)
        if "fc.weight" in need:
            _gemm_into(ws, grads["fc.weight"], D, V, D, TR, dpred, V, ws.H[1:], D, AMM, BKR, gf=gf)
        if "fc.bias" in need:
            K.colsum(dpred, TR, V, V, grads["fc.bias"], ws.work)
        # ---- backward through time
        s_dh = dm.s_dh
        S_dh = sum(s_dh)
        W_ih_awe = W_ih[:, M:]
        wf = p["attention.full_att.weight"]
        cur = 0
        for t in range(T - 1, -1, -1):
            K.lstm_cell_bwd(ws.DHD[t], ws.P_dh, S_dh if t < T - 1 else 0, R * D, ws.DC[cur] if t < T - 1 else None,
                            ws.ACT[t], ws.C[t], ws.C[t + 1], R, D, R, ws.DG[t], ws.DC[cur ^ 1])
            cur ^= 1
            K.gemm(K.problem(R, E, 4 * D, ws.DG[t], 4 * D, W_ih_awe, X, ws.P_dx, E, ksplit=dm.s_dx,
                             c_split_stride=R * E), AK, BKR, K.TILE_64, flags=gf)
            K.att_group_bwd(ws.P_dx, dm.s_dx, R * E, ws.GATE[t], ws.AWE[t], enc, ws.ALPHA[t], P, ws.ATT_ENC, ws.AD[t],
                            wf, B, n, P, A, E, ws.DALPHA, ws.DGP[t], ws.DE[t], ws.DAD[t])
            o1, o2 = s_dh[0] * R * D, (s_dh[0] + s_dh[1]) * R * D
            K.gemm([K.problem(R, D, 4 * D, ws.DG[t], 4 * D, p["decode_step.weight_hh"], D, ws.P_dh, D,
                              ksplit=s_dh[0], c_split_stride=R * D),
                    K.problem(R, D, E, ws.DGP[t], E, p["f_beta.weight"], D, ws.P_dh.view(-1)[o1:], D,
                              ksplit=s_dh[1], c_split_stride=R * D),
                    K.problem(R, D, A, ws.DAD[t], A, p["attention.dec_att.weight"], D, ws.P_dh.view(-1)[o2:], D,
                              ksplit=s_dh[2], c_split_stride=R * D)], AK, BKR, K.TILE_64, flags=gf)
        # dh0 / dc0 summed over each image's rows -> h_lin / c_lin
        K.splitk_reduce(ws.P_dh, S_dh, R * D, R, D, D, ws.DH0, D)
        K.segment_sum_rows(ws.DH0, ws.seg, B, R, D, ws.DH0G)
        K.segment_sum_rows(ws.DC[cur], ws.seg, B, R, D, ws.DC0G)
        for nm, dd in (("h_lin", ws.DH0G), ("c_lin", ws.DC0G)):
            if nm + ".weight" in need:
                K.gemm(K.problem(D, E, B, dd, D, ws.mean, E, grads[nm + ".weight"], E), AMM, BKR, K.TILE_128, flags=gf)
            if nm + ".bias" in need:
                K.colsum(dd, B, D, D, grads[nm + ".bias"], ws.work)
        # ---- hoisted weight gradients over all t
        Hprev = ws.H[:T]
        if "decode_step.weight_ih" in need:
            _gemm_into(ws, grads["decode_step.weight_ih"], X, 4 * D, X, TR, ws.DG, 4 * D, ws.X, X, AMM, BKR, gf=gf)
        if "decode_step.weight_hh" in need:
            _gemm_into(ws, grads["decode_step.weight_hh"], D, 4 * D, D, TR, ws.DG, 4 * D, Hprev, D, AMM, BKR, gf=gf)
        if "decode_step.bias_ih" in need or "decode_step.bias_hh" in need:
            tgt = grads.get("decode_step.bias_ih", grads.get("decode_step.bias_hh"))
            K.colsum(ws.DG, TR, 4 * D, 4 * D, tgt, ws.work)
            for nm in ("decode_step.bias_ih", "decode_step.bias_hh"):
                if nm in need and grads[nm] is not tgt:
                    grads[nm].copy_(tgt)
        if "f_beta.weight" in need:
            _gemm_into(ws, grads["f_beta.weight"], D, E, D, TR, ws.DGP, E, Hprev, D, AMM, BKR, gf=gf)
        if "f_beta.bias" in need:
            K.colsum(ws.DGP, TR, E, E, grads["f_beta.bias"], ws.work)
        if "attention.dec_att.weight" in need:
            _gemm_into(ws, grads["attention.dec_att.weight"], D, A, D, TR, ws.DAD, A, Hprev, D, AMM, BKR, gf=gf)
        if "attention.dec_att.bias" in need:
            K.colsum(ws.DAD, TR, A, A, grads["attention.dec_att.bias"], ws.work)
        # d(att_enc) summed over t and the group, full_att grads, then enc_att grads over the B*P rows
        nblk = K.att_group_enc_grad(ws.DE, ws.ATT_ENC, ws.AD, wf, T, B, n, P, A, ws.DATT, ws.WF_PART, ws.BF_PART)
        if "attention.full_att.weight" in need:
            K.colsum(ws.WF_PART, nblk, A, A, grads["attention.full_att.weight"], ws.work)
        if "attention.full_att.bias" in need:
            K.colsum(ws.BF_PART, nblk, 1, 1, grads["attention.full_att.bias"], ws.work)
        if "attention.enc_att.weight" in need:
            _gemm_into(ws, grads["attention.enc_att.weight"], E, A, E, B * P, ws.DATT, A, enc, E, AMM, BKR, gf=gf)
        if "attention.enc_att.bias" in need:
            K.colsum(ws.DATT, B * P, A, A, grads["attention.enc_att.bias"], ws.work)
        if "embedding.weight" in need:
            demb = grads["embedding.weight"]
            demb.zero_()
            dxe = ws.scratch[:TR * M].view(TR, M)
            K.gemm(K.problem(TR, M, 4 * D, ws.DG, 4 * D, W_ih, X, dxe, M), AK, BKR, K.TILE_128, flags=gf)
            K.embed_scatter_add(dxe, M, st["caps"], R, L, T, None, M, demb)
