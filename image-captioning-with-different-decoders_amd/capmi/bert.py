"""Frozen BERT word features for the ``use_bert`` captioner (reference models/attention.py:96-100,166-215).

``BertWeights`` loads a local bert-base-style checkpoint (never by name: nothing here touches a network);
``BertEmbedder`` is the ``decoder.bert_embedder`` callable: (B, L) int64 caption tokens -> (B, L+1, hidden)
float32 word-level features of encoder layer ``layer`` on the device. Row 0 is [CLS]; row 1+i is the SUM of
the layer outputs of word i's pieces -- what the reference's alignment loop produces whenever it converges
(when it does not -- an [UNK] piece, a word containing '#', stripped accents -- the reference drops rows and
fails in torch.stack; here the rule stays "sum of that word's pieces").

The forward is launch-only: captions are packed raggedly (one row per word piece, no padding rows), the
piece ids / positions / sequence offsets / word segment offsets of a batch come from a per-vocabulary CSR
table by vectorised numpy and go up in one buffer, and every layer is
QKV GEMM -> capmi_bert_attention -> out-proj GEMM -> capmi_add_ln -> FFN-in GEMM -> capmi_bias_gelu ->
FFN-out GEMM -> capmi_add_ln (biases in the GEMM epilogues), then capmi_segment_sum_rows writes the
(B, L+1, hidden) tensor. Activations are fp32 in every precision.

Host work per call: the caption tokens are needed on the host to size the ragged batch. Tokens that live on
the device cost one small device->host copy (a sync); pass ``host_tokens`` to avoid it.
"""
import json
import os

import numpy as np
import torch

from . import kernels as K
from ._lib import CAPMI_A_KMAJOR as AK
from ._lib import CAPMI_GEMM_BF16, CAPMI_GEMM_SPLIT3
from .text import WordPieceTokenizer, word_pieces

PRECISIONS = ("fp32-x3", "bf16", "fp32")
_PREFIXES = ("bert_model.", "bert.")
_LAYER_KEYS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
               "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")
ROW_BUCKET = 256


def required_keys(num_layers):
    keys = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
            "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for i in range(num_layers):
        for k in _LAYER_KEYS:
            keys += [f"encoder.layer.{i}.{k}.weight", f"encoder.layer.{i}.{k}.bias"]
    return keys


def normalize_key(name):
    """HF key name without the optional 'bert.' / 'bert_model.' prefix (the second is what a reference decoder
    state_dict carries: it registers BERT as a submodule), old LayerNorm.gamma / .beta -> .weight / .bias."""
    for p in _PREFIXES:
        if name.startswith(p):
            name = name[len(p):]
            break
    if name.endswith("LayerNorm.gamma"):
        name = name[:-len("gamma")] + "weight"
    elif name.endswith("LayerNorm.beta"):
        name = name[:-len("beta")] + "bias"
    return name


class BertWeights:
    """fp32 CPU tensors of a BERT encoder under the HF key names (pooler and heads dropped), its config dict
    and the path of its vocab.txt."""

    def __init__(self, tensors, config, vocab_file=None):
        self.config = dict(config)
        for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
                  "max_position_embeddings"):
            if k not in self.config:
                raise KeyError(f"BERT config lacks {k}")
        self.config.setdefault("layer_norm_eps", 1e-12)
        want = required_keys(int(self.config["num_hidden_layers"]))
        got = {}
        for name, t in tensors.items():
            n = normalize_key(name)
            if n in want:
                got[n] = t.detach().to(torch.float32).contiguous()
        missing = [k for k in want if k not in got]
        if missing:
            raise KeyError(f"BERT checkpoint lacks {len(missing)} tensors: {', '.join(missing)}")
        self.tensors = got
        self.vocab_file = vocab_file

    @classmethod
    def load(cls, path):
        """``path``: a local directory holding pytorch_model.bin (or model.safetensors when safetensors is
        importable), config.json / bert_config.json and vocab.txt, or the weights file itself in such a
        directory. A model NAME is an error: nothing is ever fetched."""
        path = os.fspath(path)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path!r} is not a local file or directory (BERT weights are never fetched "
                                    "by name: point --bert_path at a local checkpoint directory)")
        if os.path.isdir(path):
            root, wfile = path, None
            cands = ["pytorch_model.bin"]
            try:
                import safetensors  # noqa: F401
                cands.insert(0, "model.safetensors")
            except ImportError:
                pass
            for c in cands:
                if os.path.exists(os.path.join(root, c)):
                    wfile = os.path.join(root, c)
                    break
            if wfile is None:
                raise FileNotFoundError(f"no {' / '.join(cands)} in {root}")
        else:
            root, wfile = os.path.dirname(path) or ".", path
        cfg = next((os.path.join(root, c) for c in ("config.json", "bert_config.json")
                    if os.path.exists(os.path.join(root, c))), None)
        if cfg is None:
            raise FileNotFoundError(f"no config.json / bert_config.json in {root}")
        with open(cfg) as f:
            config = json.load(f)
        vocab_file = os.path.join(root, "vocab.txt")
        if not os.path.exists(vocab_file):
            raise FileNotFoundError(f"no vocab.txt in {root}")
        if wfile.endswith(".safetensors"):
            from safetensors.torch import load_file
            tensors = load_file(wfile)
        else:
            tensors = torch.load(wfile, map_location="cpu", weights_only=True)
        return cls(tensors, config, vocab_file)


def batch_layout(tokens, offsets, piece_ids, cls_id):
    """Ragged layout of a caption batch, vectorised (no per-caption loop). ``tokens`` (B, L) integer array of
    caption-vocabulary indices; ``offsets`` / ``piece_ids`` the word_pieces CSR table; each caption becomes the
    sequence [CLS] + pieces(word 0) + ... + pieces(word L-1). Returns int32 arrays: ``ids`` [rows] piece ids,
    ``pos`` [rows] position in the own sequence, ``seq_off`` [B+1] row offsets of the sequences, ``seg_off``
    [B*(L+1)+1] row offsets of the word segments (segment b*(L+1) is [CLS], b*(L+1)+1+i word i), and the
    longest sequence ``max_len``."""
    tokens = np.asarray(tokens, dtype=np.int64)
    B, L = tokens.shape
    V = len(offsets) - 1
    if tokens.size and (tokens.min() < 0 or tokens.max() >= V):
        raise IndexError("caption token outside the vocabulary")
    cnt = np.diff(offsets)
    seg_cnt = np.ones((B, L + 1), dtype=np.int64)
    seg_cnt[:, 1:] = cnt[tokens]
    seg_off = np.zeros(B * (L + 1) + 1, dtype=np.int64)
    np.cumsum(seg_cnt.ravel(), out=seg_off[1:])
    rows = int(seg_off[-1])
    seq_off = seg_off[::L + 1]
    # source index of every row in the CSR ids, with [CLS] as one extra entry at the end
    src_start = np.full((B, L + 1), len(piece_ids), dtype=np.int64)
    src_start[:, 1:] = offsets[tokens]
    ext = np.concatenate([np.asarray(piece_ids, dtype=np.int64), [cls_id]])
    r = np.arange(rows, dtype=np.int64)
    ids = ext[np.repeat(src_start.ravel() - seg_off[:-1], seg_cnt.ravel()) + r]
    seq_len = np.diff(seq_off)
    pos = r - np.repeat(seq_off[:-1], seq_len)
    return {"ids": ids.astype(np.int32), "pos": pos.astype(np.int32), "seq_off": seq_off.astype(np.int32),
            "seg_off": seg_off.astype(np.int32), "rows": rows, "max_len": int(seq_len.max()) if B else 0}


class _Linear:
    """One frozen nn.Linear weight staged for the chosen precision: the three bf16 split planes for
    CAPMI_GEMM_X3 (K % 32 == 0), else the fp32 weight with the flags of capmi_gemm_sk_ex."""

    def __init__(self, w, b, device, precision):
        w = w.to(device).contiguous()
        self.N, self.K = w.shape
        self.bias = b.to(device).contiguous()
        self.x3 = precision == "fp32-x3" and self.K % 32 == 0
        if self.x3:
            planes = torch.empty(3 * w.numel(), device=device, dtype=torch.bfloat16)
            K.split3_bf16(w, planes)
            self.w = planes
            self.flags = None
        else:
            self.w = w
            self.flags = {"fp32": 0, "fp32-x3": CAPMI_GEMM_SPLIT3, "bf16": CAPMI_GEMM_BF16}[precision]


class BertEmbedder:
    """``embedder(tokens)``: (B, L) int64 -> (B, L+1, hidden) float32 on ``device`` (see the module docstring).
    ``vocab``: the caption Vocabulary; ``weights``: BertWeights; ``precision``: 'fp32-x3' (fp32-accurate on the
    bf16 matrix cores, weights split once here), 'bf16' (operands rounded when staged) or 'fp32'."""

    graph_safe = False  # the ragged layout depends on the token values: not capturable (capmi.train_step)

    def __init__(self, vocab, weights, device, precision="fp32-x3", layer=11):
        if precision not in PRECISIONS:
            raise ValueError(precision)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("capmi BertEmbedder runs on the MI355X (HIP device only)")
        cfg = weights.config
        self.hidden, self.heads = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
        self.inter, self.max_pos = int(cfg["intermediate_size"]), int(cfg["max_position_embeddings"])
        self.eps = float(cfg["layer_norm_eps"])
        nl = int(cfg["num_hidden_layers"])
        if not 0 <= layer < nl:
            raise ValueError(f"layer {layer} outside 0..{nl - 1}")
        if self.hidden % self.heads:
            raise ValueError("hidden_size is not a multiple of num_attention_heads")
        self.head_dim = self.hidden // self.heads
        self.layer, self.precision, self.device = layer, precision, device
        if weights.vocab_file is None:
            raise ValueError("BertWeights has no vocab.txt")
        self.tokenizer = WordPieceTokenizer(weights.vocab_file)
        self.offsets, self.piece_ids = word_pieces(vocab, self.tokenizer)
        self.cls_id = self.tokenizer.vocab["[CLS]"]
        t = weights.tensors
        dev = lambda n: t[n].to(device).contiguous()  # noqa: E731
        self.word_emb = dev("embeddings.word_embeddings.weight")
        self.pos_emb = dev("embeddings.position_embeddings.weight")
        self.type_emb = dev("embeddings.token_type_embeddings.weight")
        self.emb_g, self.emb_b = dev("embeddings.LayerNorm.weight"), dev("embeddings.LayerNorm.bias")
        if self.piece_ids.size and int(self.piece_ids.max()) >= self.word_emb.shape[0]:
            raise ValueError("vocab.txt has more pieces than the word embedding table has rows")
        self.layers = []
        for i in range(layer + 1):  # layers above `layer` are never run: not even uploaded
            p = f"encoder.layer.{i}."
            qkv_w = torch.cat([t[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value")], 0)
            qkv_b = torch.cat([t[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value")], 0)
            lin = lambda n: _Linear(t[p + n + ".weight"], t[p + n + ".bias"], device, precision)  # noqa: E731
            self.layers.append({
                "qkv": _Linear(qkv_w, qkv_b, device, precision), "proj": lin("attention.output.dense"),
                "ln1": (dev(p + "attention.output.LayerNorm.weight"), dev(p + "attention.output.LayerNorm.bias")),
                "ffn_in": lin("intermediate.dense"), "ffn_out": lin("output.dense"),
                "ln2": (dev(p + "output.LayerNorm.weight"), dev(p + "output.LayerNorm.bias"))})
        self.sk = K.gemm_workspace(device)
        self._ws = {}
        self._idx = {}
        self.last_layout = None

    # ------------------------------------------------------------------ host side
    def layout(self, tokens):
        lay = batch_layout(tokens, self.offsets, self.piece_ids, self.cls_id)
        if lay["max_len"] > self.max_pos:
            raise ValueError(f"a caption has {lay['max_len']} word pieces; this BERT has "
                             f"{self.max_pos} position embeddings")
        return lay

    def _workspace(self, rows):
        cap = -(-rows // ROW_BUCKET) * ROW_BUCKET
        ws = self._ws.get(cap)
        if ws is None:
            f = dict(device=self.device, dtype=torch.float32)
            H = self.hidden
            ws = self._ws[cap] = {"x": torch.empty(cap, H, **f), "y": torch.empty(cap, H, **f),
                                  "t": torch.empty(cap, H, **f), "ctx": torch.empty(cap, H, **f),
                                  "qkv": torch.empty(cap, 3 * H, **f), "ffn": torch.empty(cap, self.inter, **f)}
        return cap, ws

    def _gemm(self, M, A, lin, C):
        prob = K.problem(M, lin.N, lin.K, A, lin.K, lin.w, lin.K, C, lin.N, bias=lin.bias)
        if lin.x3:
            K.gemm_x3(prob, AK, self.sk)
        else:
            K.gemm_sk(prob, AK, self.sk, K.TILE_AUTO, flags=lin.flags)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def __call__(self, tokens, out=None, host_tokens=None):
        if host_tokens is None:
            host_tokens = tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else np.asarray(tokens)
        elif isinstance(host_tokens, torch.Tensor):
            host_tokens = host_tokens.numpy()
        B, L = host_tokens.shape
        lay = self.layout(host_tokens)
        self.last_layout = lay
        rows, nseg, H = lay["rows"], B * (L + 1), self.hidden
        cap, ws = self._workspace(rows)
        key = (cap, B, L)
        idx = self._idx.get(key)
        if idx is None:
            idx = self._idx[key] = torch.empty(2 * cap + (B + 1) + (nseg + 1), device=self.device, dtype=torch.int32)
        packed = np.zeros(idx.numel(), dtype=np.int32)
        packed[:rows] = lay["ids"]
        packed[cap:cap + rows] = lay["pos"]
        packed[2 * cap:2 * cap + B + 1] = lay["seq_off"]
        packed[2 * cap + B + 1:] = lay["seg_off"]
        idx.copy_(torch.from_numpy(packed))  # one upload (pageable source: reusable on return)
        ids, pos = idx[:cap], idx[cap:2 * cap]
        seq_off, seg_off = idx[2 * cap:2 * cap + B + 1], idx[2 * cap + B + 1:]
        if out is None:
            out = torch.empty(B, L + 1, H, device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (B, L + 1, H) or not out.is_contiguous():
            raise ValueError("out must be a contiguous (B, L+1, hidden) tensor")

        x, y = ws["x"], ws["y"]
        K.bert_embed_ln(self.word_emb, self.pos_emb, self.type_emb, ids, pos, rows, self.emb_g, self.emb_b,
                        self.eps, x)
        for lyr in self.layers:
            self._gemm(rows, x, lyr["qkv"], ws["qkv"])
            K.bert_attention(ws["qkv"], seq_off, B, rows, lay["max_len"], self.heads, self.head_dim, ws["ctx"])
            self._gemm(rows, ws["ctx"], lyr["proj"], ws["t"])
            K.add_ln(ws["t"], None, x, rows, H, lyr["ln1"][0], lyr["ln1"][1], self.eps, y)
            self._gemm(rows, y, lyr["ffn_in"], ws["ffn"])
            K.bias_gelu(ws["ffn"], None, rows, self.inter)
            self._gemm(rows, ws["ffn"], lyr["ffn_out"], ws["t"])
            K.add_ln(ws["t"], None, y, rows, H, lyr["ln2"][0], lyr["ln2"][1], self.eps, x)
        K.segment_sum_rows(x, seg_off, nseg, rows, H, out)
        return out


def build_embedder(decoder, bert_path, device):
    """The BertEmbedder of ``decoder`` (its vocabulary and compute_precision) from a local checkpoint: layer 11
    (reference :179), or the last layer of a checkpoint with fewer than 12."""
    weights = BertWeights.load(bert_path)
    return BertEmbedder(decoder.vocab, weights, device, precision=getattr(decoder, "compute_precision", "fp32"),
                        layer=min(11, int(weights.config["num_hidden_layers"]) - 1))
