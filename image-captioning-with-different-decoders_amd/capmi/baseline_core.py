"""The baseline (LSTM) decoder's recurrence on libcapmi, defined once: one step, the teacher-forced forward
and the backward through time (the counterpart of capmi.decoder_core for the attention decoder).

The model is reference models/baseline.py:24-111: an LSTM over [image feature, embedding(captions[:, :-1])],
then Linear to the vocabulary. The input half of the LSTM GEMM is hoisted over all T steps (one (T*B) x 4H x M
GEMM, both LSTM biases in its epilogue); each step adds h_{t-1} W_hh^T and runs the cell (gate order i,f,g,o as
torch.nn.LSTM), in one launch (``fused``) or as capmi_gemm TILE_64 + capmi_lstm_cell_fwd; the vocabulary
projection is one (T*B) x V x H GEMM written batch-first (row remap) after the loop. The backward is BPTT on
capmi_lstm_step_bwd (``fused``) or capmi_lstm_cell_bwd + the recurrent dh GEMM per step, hoisted weight
gradients and the embedding scatter-add. State is time-major: X[t][b][M], H[t][b][H], C, ACT[t][b][4H].

Callers: capmi.baseline_fn (autograd, unfused), capmi.baseline_eval (validation), capmi.baseline_train (the
training step) and capmi.rollout.BaselineStepper (beam search and sampling, through ``step``).
"""
import torch

from . import kernels as K
from ._lib import CAPMI_A_KMAJOR, CAPMI_A_MMAJOR, CAPMI_B_KROWS, CAPMI_B_NMAJOR_W

AK, AMM, BW, BKR = CAPMI_A_KMAJOR, CAPMI_A_MMAJOR, CAPMI_B_NMAJOR_W, CAPMI_B_KROWS
PNAMES = ("embedding.weight", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
          "linear.weight", "linear.bias")


def params(dec):
    """The decoder's parameters in PNAMES order."""
    lstm = dec.lstm
    return (dec.embedding.weight, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0,
            dec.linear.weight, dec.linear.bias)


def check_inputs(img_features, captions=None):
    """What every baseline path asks of its inputs."""
    if not (img_features.is_cuda and (captions is None or captions.is_cuda)):
        raise RuntimeError("capmi baseline decoder path needs HIP tensors")
    if captions is not None and captions.dtype != torch.int64:
        raise TypeError("captions must be int64")


def step(p, R, M, H, h_out, c_out, pre=None, x=None, ld_x=0, h_prev=None, c_prev=None, scratch=None, fused=True,
         act_out=None):
    """One LSTM step over R rows on the parameters ``p`` (``params``): ``pre`` (R, 4H) already holds the input
    product and the biases, or ``x`` (R, M) is multiplied here. ``act_out`` (R, 4H) receives the gate
    activations the backward needs. ``fused``: one launch (capmi_lstm_step_fwd, capmi_lstm_step_fwd_train with
    ``act_out``). Otherwise the sequence it stands for, on ``scratch``, (4, R, 4H) or four buffers: the two GEMM
    products, zeros for a missing c_prev (written here) and the cell kernel's activation output when there is
    no ``act_out``."""
    if fused:
        _, w_ih, w_hh, b_ih, b_hh, _, _ = p
        kw = dict(pre=pre, x=x, ld_x=ld_x, h_prev=h_prev, c_prev=c_prev, w_ih=w_ih if x is not None else None,
                  w_hh=w_hh if h_prev is not None else None, b_ih=b_ih if pre is None else None,
                  b_hh=b_hh if pre is None else None)
        if act_out is None:
            K.lstm_step_fwd(R, M, H, h_out, c_out, **kw)
        else:
            K.lstm_step_fwd_train(R, M, H, h_out, c_out, act_out, **kw)
        return
    if x is not None:
        pre = scratch[0]
        K.gemm(K.problem(R, 4 * H, M, x, ld_x or M, p[1], M, pre, 4 * H, bias=p[3], bias2=p[4]), AK, BW, K.TILE_64)
    if c_prev is None:
        c_prev = scratch[2].view(-1)[:R * H].zero_()
    if act_out is None:
        act_out = scratch[3]
    if h_prev is None:
        K.lstm_cell_fwd(pre, 1, 0, None, None, 0, 0, c_prev, R, H, h_out, c_out, act_out)
        return
    hh = scratch[1]
    K.gemm(K.problem(R, 4 * H, H, h_prev, H, p[2], H, hh, 4 * H), AK, BW, K.TILE_64)
    K.lstm_cell_fwd(pre, 1, 0, None, hh, 1, 0, c_prev, R, H, h_out, c_out, act_out)


def forward(dec, caps, X, GX, H, C, logits, ACT=None, fused=True, scratch=None):
    """Teacher-forced forward over caps (B, L) int64, T = L steps. X (T, B, M) holds the image feature in X[0];
    steps 1.. are gathered here. GX (T*B, 4H), H, C (T, B, H) and ACT (T, B, 4H; None: not kept) are written,
    then logits (B, T, V). ``fused`` False needs ``scratch`` = (unused, (B, 4H), (B, H) zeros the caller keeps
    zero, (B, 4H) when ACT is None)."""
    p = emb_w, w_ih, _, b_ih, b_hh, w_lin, b_lin = params(dec)
    B, L = caps.shape
    T, M, Hd, V = L, dec.embed_size, dec.hidden_size, w_lin.shape[0]
    sk = dec._capmi_ws(caps.device)
    if T > 1:  # steps 1.. = embedding(captions[:, :-1]) (reference :98-101)
        K.embed_gather(emb_w, caps, B, L, T - 1, X[1:], M)
    K.gemm_sk(K.problem(T * B, 4 * Hd, M, X, M, w_ih, M, GX, 4 * Hd, bias=b_ih, bias2=b_hh), AK, sk, K.TILE_AUTO)
    # the fused kernels take a missing c_prev; the cell kernel reads the caller's zeros
    h_prev, c_prev = None, None if fused else scratch[2]
    for t in range(T):
        h, c = H[t], C[t]
        step(p, B, M, Hd, h, c, GX[t * B:], None, 0, h_prev, c_prev, scratch, fused, None if ACT is None else ACT[t])
        h_prev, c_prev = h, c
    # row r = t*B + b of the (T*B, V) product lands at logits[b][t]: remap (r % B)*T*V + (r / B)*V
    K.gemm_sk(K.problem(T * B, V, Hd, H, Hd, w_lin, Hd, logits, T * V, c_r1=B, c_s2=V, bias=b_lin), AK, sk,
              K.TILE_AUTO)


def backward(dec, caps, ws, dlogits, grads, dlogits_time_major=False, fused=False, need_dx=False):
    """Writes parameter gradients into ``grads`` (PNAMES name -> pre-allocated tensor; a name left out is not
    computed). ``ws``: X, H, C, ACT as ``forward`` left them and the scratch dH (T*B, H), DG (T, B, 4H), DHR
    (B, H), DC (two of (B, H)), DX (T, B, M), gb (4H), cs_v / cs_g (colsum work for V / 4H columns), zeros
    (B, H). dlogits: the gradient of the logits, batch-first (B, T, V), or (T*B, V) with row t*B + b when
    ``dlogits_time_major``. ``need_dx``: ws.DX = d(loss)/dX also when no embedding gradient asks for it (DX[0]
    is the image feature's)."""
    emb_w, w_ih, w_hh, _, _, w_lin, _ = params(dec)
    B, L = caps.shape
    T, M, Hd, V = L, dec.embed_size, dec.hidden_size, w_lin.shape[0]
    sk = dec._capmi_ws(caps.device)
    # A rows of the (T*B, V) operand: remapped from batch-first, or as they lie
    ar, lda = (dict(), V) if dlogits_time_major else (dict(a_r1=B, a_s2=V), T * V)
    K.gemm_sk(K.problem(T * B, Hd, V, dlogits, lda, w_lin, Hd, ws.dH, Hd, **ar), AK, sk, K.TILE_AUTO, bmode=BKR)
    if "linear.weight" in grads:  # dW_lin = dlogits^T H over the (T*B) rows
        K.gemm_sk(K.problem(V, Hd, T * B, dlogits, lda, ws.H, Hd, grads["linear.weight"], Hd, **ar), AMM, sk,
                  K.TILE_AUTO, bmode=BKR)
    if "linear.bias" in grads:
        K.colsum(dlogits, T * B, V, V, grads["linear.bias"], ws.cs_v)
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        dh_lin = ws.dH[t * B:(t + 1) * B]
        dc_in = None if last else ws.DC[(t + 1) & 1]
        if fused:
            K.lstm_step_bwd(B, Hd, ws.ACT[t], ws.C[t], ws.DG[t], ws.DC[t & 1], dh_lin=dh_lin,
                            dg_next=None if last else ws.DG[t + 1], w_hh=w_hh, dc_in=dc_in,
                            c_prev=ws.C[t - 1] if t > 0 else None)
            continue
        if not last:  # dh_t (recurrent part) = dgates_{t+1} . W_hh
            K.gemm(K.problem(B, Hd, 4 * Hd, ws.DG[t + 1], 4 * Hd, w_hh, Hd, ws.DHR, Hd), AK, BKR, K.TILE_64)
        K.lstm_cell_bwd(dh_lin, ws.DHR, 0 if last else 1, 0, dc_in, ws.ACT[t], ws.C[t - 1] if t > 0 else ws.zeros,
                        ws.C[t], B, Hd, B, ws.DG[t], ws.DC[t & 1])
    if "lstm.weight_ih_l0" in grads:  # dW_ih = DG^T X
        K.gemm_sk(K.problem(4 * Hd, M, T * B, ws.DG, 4 * Hd, ws.X, M, grads["lstm.weight_ih_l0"], M), AMM, sk,
                  K.TILE_AUTO, bmode=BKR)
    if "lstm.weight_hh_l0" in grads:
        if T > 1:  # dW_hh = sum_{t>=1} DG[t]^T H[t-1]
            K.gemm_sk(K.problem(4 * Hd, Hd, (T - 1) * B, ws.DG[1:], 4 * Hd, ws.H, Hd, grads["lstm.weight_hh_l0"], Hd),
                      AMM, sk, K.TILE_AUTO, bmode=BKR)
        else:
            grads["lstm.weight_hh_l0"].zero_()
    if "lstm.bias_ih_l0" in grads or "lstm.bias_hh_l0" in grads:
        K.colsum(ws.DG, T * B, 4 * Hd, 4 * Hd, ws.gb, ws.cs_g)
        for nm in ("lstm.bias_ih_l0", "lstm.bias_hh_l0"):
            if nm in grads:
                grads[nm].copy_(ws.gb)
    g_emb = grads.get("embedding.weight")
    if need_dx or (g_emb is not None and T > 1):
        # dX = DG . W_ih: step 0 -> the image feature, steps 1.. -> the embedding rows
        K.gemm_sk(K.problem(T * B, M, 4 * Hd, ws.DG, 4 * Hd, w_ih, M, ws.DX, M), AK, sk, K.TILE_AUTO, bmode=BKR)
    if g_emb is not None:
        g_emb.zero_()
        if T > 1:
            K.embed_scatter_add(ws.DX[1:], M, caps, B, L, T - 1, None, M, g_emb)
