"""One 'baseline' (LSTM captioner) training step on the MI355X (reference models/baseline.py:114-264).

    x0 = embed(resnet(imgs))                       frozen ResNet-101 + the embed Linear
    decoder forward (capmi.baseline_core)          embed_gather, hoisted (T B) x 4H x M GEMM with both biases,
                                                   T x capmi_lstm_step_fwd_train, hoisted vocabulary GEMM
    loss = CrossEntropyLoss(ignore_index=PAD)      capmi_count_targets, capmi_ce_ignore_fwd_bwd (time-major
                                                   dlogits), capmi_loss_finalize_dev: the count stays on the device
    backward (capmi.baseline_core)                 dH / dW_lin / db_lin, T x capmi_lstm_step_bwd, hoisted dW_ih,
                                                   dW_hh, bias column sums, dX, embedding scatter-add
    grads <- all-reduce mean over ranks            (DP only)
    params <- clamp(+-grad_clip) + Adam            capmi.optim.Adam: one kernel, step count on the device

Every parameter gradient is written in place into the ``p.grad`` views of the optimizer's flat buffer; every
workspace is allocated once per (batch, caption) shape. ``graph=True`` captures the whole step once per shape
into a HIP graph (torch.cuda.CUDAGraph) and replays it: inputs are copied into static buffers, the chain is
linear. With more than one rank the graph ends after the backward; the all-reduce and the update run eagerly
after it (capmi.train_step's convention: the mean over ranks of per-rank mean losses' gradients).

Parameters follow ``requires_grad`` as capmi.baseline_fn does (frozen embedding by default, fp64 GloVe table).
With ``encoder_optimizer`` the encoder's ``embed`` Linear trains (the reference builds that optimizer over the
encoder's trainable parameters only): dW_embed = dX[0]^T feats, db_embed = colsum(dX[0]), its own Adam. Without
it d(image features) is not computed.

The loss is returned as a device tensor (1,), no host sync; it is the step's own buffer, overwritten by the next
call of the same shape: clone it to keep it.

STEP_FUSED_FWD / STEP_FUSED_BWD: one launch per timestep (capmi_lstm_step_fwd_train / capmi_lstm_step_bwd), or
the sequence they stand for (capmi_gemm TILE_64 with capmi_lstm_cell_fwd / capmi_lstm_cell_bwd) when False.
"""
import os
import types

import torch

from . import baseline_core as core
from . import dist as cdist
from . import kernels as K
from .baseline_core import AK, AMM, BKR, BW
STEP_FUSED_FWD = True
STEP_FUSED_BWD = True


class BaselineTrainStep:
    def __init__(self, encoder, decoder, optimizer, ctx=None, graph=False, encoder_optimizer=None, ignore_index=0):
        for opt in (optimizer, encoder_optimizer):
            if opt is not None and not hasattr(opt, "grad_buffers"):
                raise TypeError("BaselineTrainStep needs capmi.optim.Adam (gradients live in its flat buffer)")
        self.encoder, self.decoder, self.opt, self.enc_opt = encoder, decoder, optimizer, encoder_optimizer
        dev = next(decoder.parameters()).device
        self.ctx = ctx or cdist.DistCtx(device=dev)
        self.ignore_index = int(ignore_index)
        self.graph_mode = graph
        self.fused_fwd, self.fused_bwd = STEP_FUSED_FWD, STEP_FUSED_BWD
        self.train_embed = encoder_optimizer is not None
        if self.train_embed:
            if not hasattr(encoder, "pooled_features"):
                raise NotImplementedError("a trainable encoder needs pooled_features() and an embed Linear")
            owned = {id(q) for grp in encoder_optimizer.param_groups for q in grp["params"]}
            if not owned <= {id(q) for q in encoder.embed.parameters()}:
                raise NotImplementedError("capmi: only the Encoder's embed Linear trains on this path")
        self._ws = {}      # (B, L) -> buffers of that shape
        self._gcache = {}  # (image shape, caption shape) -> (graph, static inputs); no eviction
        self.graph_cache_size = int(os.environ.get("CAPMI_GRAPH_CACHE", "8"))
        self.counts = {"replay": 0, "eager": 0, "capture": 0}
        self.capture_error_mode = "global"  # "thread_local" beside a DataLoader's pin-memory thread (AttentionTrainStep)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, B, L):
        ws = self._ws.get((B, L))
        if ws is not None:
            return ws
        dec = self.decoder
        T, M, Hd, V = L, dec.embed_size, dec.hidden_size, dec.linear.weight.shape[0]
        dev = dec.linear.weight.device
        e = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
        ws = types.SimpleNamespace(
            X=e(T, B, M), GX=e(T * B, 4 * Hd), H=e(T, B, Hd), C=e(T, B, Hd), ACT=e(T, B, 4 * Hd), HH=e(B, 4 * Hd),
            zeros=torch.zeros(B, Hd, device=dev), logits=e(B, T, V), dlogits=e(T * B, V), loss_rows=e(B * T),
            count=torch.zeros(1, dtype=torch.int32, device=dev), inv=e(1), loss=e(1), dH=e(T * B, Hd),
            DG=e(T, B, 4 * Hd), DHR=e(B, Hd), DC=[e(B, Hd), e(B, Hd)], DX=e(T, B, M),
            cs_v=e(K.colsum_work_size(T * B, V)), cs_g=e(K.colsum_work_size(T * B, 4 * Hd)),
            cs_m=e(K.colsum_work_size(B, M)), gb=e(4 * Hd))
        self._ws[(B, L)] = ws
        return ws

    # ------------------------------------------------------------------ the step
    def _encode(self, imgs, ws):
        """Step 0 of the decoder's input, ws.X[0] = embed(resnet(imgs)); returns the pooled features when the
        embed Linear trains (its weight gradient needs them)."""
        enc = self.encoder
        if not hasattr(enc, "pooled_features"):  # any frozen module producing (B, M) features
            with torch.no_grad():
                ws.X[0].copy_(enc(imgs).float())
            return None
        with torch.no_grad():
            feats = enc.pooled_features(imgs)
        N, F = feats.shape
        M = enc.embed.out_features
        K.gemm(K.problem(N, M, F, feats, F, enc.embed.weight, F, ws.X[0], M, bias=enc.embed.bias), AK, BW, K.TILE_64)
        return feats

    def _forward(self, caps, ws):
        B, T = caps.shape
        core.forward(self.decoder, caps, ws.X, ws.GX, ws.H, ws.C, ws.logits, ws.ACT, fused=self.fused_fwd,
                     scratch=(None, ws.HH, ws.zeros, None))
        K.count_targets(caps, B, T, T, 0, self.ignore_index, ws.count, ws.inv)
        K.ce_ignore_fwd_bwd(ws.logits, caps, B, T, T, ws.logits.shape[2], 0, self.ignore_index, ws.inv, ws.loss_rows,
                            ws.dlogits, True)
        K.loss_finalize_dev(ws.loss_rows, B * T, ws.inv, ws.loss)

    def _backward(self, caps, ws, feats):
        dec = self.decoder
        grads = {n: q.grad for n, q in zip(core.PNAMES, core.params(dec)) if q.requires_grad}
        # ws.dlogits is time-major (T*B, V), row t*B + b: the rows of H
        core.backward(dec, caps, ws, ws.dlogits, grads, dlogits_time_major=True, fused=self.fused_bwd,
                      need_dx=self.train_embed)
        if self.train_embed:
            emb = self.encoder.embed
            B, M, F = caps.shape[0], dec.embed_size, feats.shape[1]
            sk = dec._capmi_ws(caps.device)
            if emb.weight.requires_grad:  # dW_embed = dX[0]^T feats
                K.gemm_sk(K.problem(M, F, B, ws.DX[0], M, feats, F, emb.weight.grad, F), AMM, sk, K.TILE_AUTO,
                          bmode=BKR)
            if emb.bias is not None and emb.bias.requires_grad:
                K.colsum(ws.DX[0], B, M, M, emb.bias.grad, ws.cs_m)

    def _step_all(self):
        self.opt.step()
        if self.enc_opt is not None:
            self.enc_opt.step()

    def _grad_buffers(self):
        bufs = list(self.opt.grad_buffers())
        if self.enc_opt is not None:
            bufs += list(self.enc_opt.grad_buffers())
        return bufs

    def _body(self, imgs, caps, with_update):
        B, L = caps.shape
        ws = self._buffers(B, L)
        feats = self._encode(imgs, ws)
        self._forward(caps, ws)
        self._backward(caps, ws, feats)
        if with_update:
            self._step_all()
        return ws.loss

    def _finish_dp(self):
        cdist.allreduce_mean_(self._grad_buffers(), self.ctx)
        self._step_all()

    # ------------------------------------------------------------------ launch modes
    def __call__(self, imgs, captions, update=True):
        """One step; returns the loss (device tensor (1,), no host sync). ``update=False`` (eager): gradients
        only, left in the optimizer's flat buffer."""
        if not (imgs.is_cuda and captions.is_cuda):
            raise RuntimeError("BaselineTrainStep needs HIP tensors")
        if captions.dtype != torch.int64:
            raise TypeError("captions must be int64")
        captions = captions.contiguous()
        if self.graph_mode and update:
            return self._replay(imgs, captions)
        return self._eager(imgs, captions, update)

    def _eager(self, imgs, captions, update=True):
        self.counts["eager"] += 1
        dp = self.ctx.distributed
        loss = self._body(imgs, captions, with_update=update and not dp)
        if update and dp:
            self._finish_dp()
        return loss

    def _replay(self, imgs, captions):
        key = (tuple(imgs.shape), tuple(captions.shape))
        ent = self._gcache.get(key)
        if ent is None:
            if len(self._gcache) >= self.graph_cache_size:
                return self._eager(imgs, captions)  # cache full: this shape runs eagerly
            ent = self._gcache[key] = self._capture(imgs, captions)
        graph, st = ent
        self.counts["replay"] += 1
        if imgs.data_ptr() != st["imgs"].data_ptr():
            st["imgs"].copy_(imgs, non_blocking=True)
        if captions.data_ptr() != st["caps"].data_ptr():
            st["caps"].copy_(captions, non_blocking=True)
        graph.replay()
        if self.ctx.distributed:
            self._finish_dp()
        return st["loss"]

    def _capture(self, imgs, captions, warmup=2):
        st = {"imgs": imgs.detach().clone(), "caps": captions.detach().clone()}
        # warm-up on a side stream: every workspace is allocated outside the graph's pool. No update (the
        # gradients are overwritten by the next step); the BatchNorm buffers a train-mode encoder forward
        # advances are restored, so a replay sequence equals the eager one.
        snap = [(b, b.detach().clone()) for b in self.encoder.buffers()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._body(st["imgs"], st["caps"], with_update=False)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        with torch.no_grad():
            for b, v in snap:
                b.copy_(v)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=self.capture_error_mode):
            st["loss"] = self._body(st["imgs"], st["caps"], with_update=not self.ctx.distributed)
        # the encoder runner's per-shape workspace cache keeps only the latest shape: hold this one's
        st["pins"] = [getattr(getattr(self.encoder, "_runner", None), "_ws", None), self._ws[tuple(captions.shape)]]
        self.counts["capture"] += 1
        return g, st
