"""Cost of the real BERT word features (capmi.bert.BertEmbedder) at the flagship shape: B = 64 captions of
L = 25 tokens over synthetic_vocab(8100), random weights of bert-base geometry (12 layers, hidden 768, 12 heads,
3072, 30522 x 768 word table), layer 11.

Arms, all in one process on one GPU, warmed up, then run in turn --repeats times (host clock around --calls
calls ending in a device synchronise; the median and every repeat are reported):

  embedder fp32-x3 / bf16 / fp32   ms per BertEmbedder call (host preparation + upload + launches + kernels)
  host prep                        ms of the host-side ragged layout alone (no GPU)
  torch ops                        the same forward written with torch ops on the GPU over a PADDED batch (fp32):
                                   what a user would plug into decoder.bert_embedder without this package's kernels
  config-5 step                    AttentionTrainStep (pipelined HIP-graph mode, as train() runs it), bf16 encoder and
                                   decoder, images/s with the real embedder (bf16) and with SyntheticBertEmbedder

The synthetic vocabulary's words are 'w<digits>': a WordPiece vocab.txt with 'w' and '##0'..'##9' splits each
into 2-5 pieces, so a 25-token caption is about 120 pieces (COCO captions: about 30). --pieces-per-word 1 adds
every 'w<digits>' word to vocab.txt as a single piece (about 32 pieces per caption, the COCO-like load).

python tools/bert_bench.py [--repeats 5] [--calls 20] [--steps 30] [--pieces-per-word 1] [--out profiles/bert_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-captioning-with-different-decoders_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
            max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)
WORD_TABLE = 30522


def write_vocab(dirname, V, single_piece):
    pieces = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "<", ">", "pad", "start", "end", "unk", "w"]
    pieces += [f"##{d}" for d in range(10)]
    if single_piece:
        pieces += [f"w{i}" for i in range(V - 4)]
    path = os.path.join(dirname, "vocab.txt")
    with open(path, "w") as f:
        f.write("\n".join(pieces) + "\n")
    return path


class TorchOpsEmbedder:
    """The same features with torch ops over a padded (B, Smax) batch, fp32 (key-padding mask in the softmax)."""

    def __init__(self, emb, weights, device):
        self.emb, self.dev = emb, device
        t = weights.tensors
        self.t = {k: v.to(device) for k, v in t.items() if not k.startswith("encoder.layer.")
                  or int(k.split(".")[2]) <= emb.layer}
        self.cfg = weights.config

    @torch.no_grad()
    def __call__(self, tokens, host_tokens=None):
        host = tokens.cpu().numpy() if host_tokens is None else host_tokens
        lay = self.emb.layout(host)
        B, L = host.shape
        H, nh, eps = self.cfg["hidden_size"], self.cfg["num_attention_heads"], self.cfg["layer_norm_eps"]
        S, rows = lay["max_len"], lay["rows"]
        seq_of_row = np.repeat(np.arange(B), np.diff(lay["seq_off"]))
        flat = seq_of_row * S + lay["pos"]  # padded slot of every packed row
        ids = np.zeros(B * S, dtype=np.int64)
        ids[flat] = lay["ids"]
        valid = np.zeros(B * S, dtype=bool)
        valid[flat] = True
        seg_of_row = np.repeat(np.arange(B * (L + 1)), np.diff(lay["seg_off"]))
        dev = self.dev
        ids_d = torch.from_numpy(ids).to(dev).view(B, S)
        mask = torch.from_numpy(valid).to(dev).view(B, 1, 1, S)
        flat_d, seg_d = torch.from_numpy(flat).to(dev), torch.from_numpy(seg_of_row).to(dev)
        T = self.t
        x = (T["embeddings.word_embeddings.weight"][ids_d] + T["embeddings.position_embeddings.weight"][:S]
             + T["embeddings.token_type_embeddings.weight"][0])
        x = F.layer_norm(x, (H,), T["embeddings.LayerNorm.weight"], T["embeddings.LayerNorm.bias"], eps)
        bias = torch.zeros(B, 1, 1, S, device=dev).masked_fill_(~mask, float("-inf"))
        for i in range(self.emb.layer + 1):
            p = f"encoder.layer.{i}."
            lin = lambda z, n: F.linear(z, T[p + n + ".weight"], T[p + n + ".bias"])  # noqa: E731
            q, k, v = (lin(x, f"attention.self.{n}").view(B, S, nh, H // nh).transpose(1, 2)
                       for n in ("query", "key", "value"))
            a = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(H // nh) + bias, dim=-1) @ v
            a = lin(a.transpose(1, 2).reshape(B, S, H), "attention.output.dense")
            x = F.layer_norm(a + x, (H,), T[p + "attention.output.LayerNorm.weight"],
                             T[p + "attention.output.LayerNorm.bias"], eps)
            f = lin(F.gelu(lin(x, "intermediate.dense")), "output.dense")
            x = F.layer_norm(f + x, (H,), T[p + "output.LayerNorm.weight"], T[p + "output.LayerNorm.bias"], eps)
        out = torch.zeros(B * (L + 1), H, device=dev)
        out.index_add_(0, seg_d, x.view(B * S, H)[flat_d])
        return out.view(B, L + 1, H)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "repeats": [round(x, 4) for x in xs]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--caption-len", type=int, default=25)
    ap.add_argument("--vocab", type=int, default=8100)
    ap.add_argument("--layers", type=int, default=12, help="BERT layers (the feature layer is the last)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pieces-per-word", type=int, default=0, choices=[0, 1],
                    help="1: every vocabulary word is one piece (COCO-like piece counts); 0: 'w' + digit pieces")
    ap.add_argument("--no-step", action="store_true", help="skip the config-5 training-step arms")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bert_bench needs the GPU (no fallback)")
    dev = torch.device("cuda")

    import bert_cases as BC
    from capmi.bert import BertEmbedder, BertWeights
    from capmi.data import SyntheticBertEmbedder, synthetic_batch
    from vocabulary import synthetic_vocab

    cfg = dict(BASE, num_hidden_layers=args.layers)
    vocab = synthetic_vocab(args.vocab)
    tmp = tempfile.mkdtemp(prefix="bert_bench_")
    weights = BertWeights(BC.random_tensors(cfg, WORD_TABLE, 11), cfg, write_vocab(tmp, args.vocab, args.pieces_per_word))
    B, L = args.batch, args.caption_len
    imgs, caps, lens = synthetic_batch(B, L, args.vocab, dev, seed=1234)
    host = caps.cpu().numpy()

    res = {"shape": {"B": B, "L": L, "V": args.vocab, "layers": args.layers}, "device": torch.cuda.get_device_name(0)}
    embs = {p: BertEmbedder(vocab, weights, dev, precision=p, layer=args.layers - 1) for p in ("fp32-x3", "bf16", "fp32")}
    lay = embs["fp32"].layout(host)
    res["shape"].update(rows=lay["rows"], max_len=lay["max_len"], padded_rows=B * lay["max_len"])
    torch_arm = TorchOpsEmbedder(embs["fp32"], weights, dev)
    arms = {f"embedder {p}": (lambda e=e: e(caps)) for p, e in embs.items()}
    arms["torch ops fp32 (padded)"] = lambda: torch_arm(caps)
    # same features? (the padded torch forward against the packed HIP one, fp32)
    d = (torch_arm(caps) - embs["fp32"](caps)).abs().max()
    res["max_abs_diff_torch_vs_hip_fp32"] = float(d)
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in arms}
    prep = []
    for _ in range(args.repeats):
        for k, fn in arms.items():
            times[k].append(timed(fn, args.calls))
        t0 = time.perf_counter()
        for _ in range(args.calls):
            embs["fp32"].layout(host)
        prep.append((time.perf_counter() - t0) / args.calls * 1e3)
    res["ms_per_call"] = {k: summary(v) for k, v in times.items()}
    res["ms_host_prep"] = summary(prep)
    for k, v in res["ms_per_call"].items():
        print(json.dumps({"arm": k, "ms_per_call": v}))
    print(json.dumps({"arm": "host prep (layout only)", "ms": res["ms_host_prep"]}))

    if not args.no_step:
        from capmi.optim import Adam
        from capmi.train_step import AttentionTrainStep
        from models.attention import AttentionDecoder, AttentionDecoderParams
        from models.encoder import EncoderAttention
        del embs["fp32-x3"], embs["fp32"], torch_arm, arms
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        encoder = EncoderAttention().to(dev).train()
        encoder.set_compute_precision("bf16")
        prm = AttentionDecoderParams()
        prm.vocab, prm.embed_size, prm.use_bert = vocab, 768, True
        decoder = AttentionDecoder(dev, prm)
        decoder.set_compute_precision("bf16")
        decoder = decoder.to(dev).train()
        decoder.fine_tune_embeddings(False)
        opt = Adam(filter(lambda q: q.requires_grad, decoder.parameters()), lr=1e-4)
        opt.set_clip(5.0)
        embedders = {"real BertEmbedder bf16": embs["bf16"],
                     "SyntheticBertEmbedder": SyntheticBertEmbedder(args.vocab, 768, device=dev)}
        steps = {}
        for k, e in embedders.items():
            decoder.bert_embedder = e
            steps[k] = AttentionTrainStep(encoder, decoder, opt, None, alpha_c=1.0, graph=True, seed=77, pipeline=True)
            for _ in range(args.warmup + 2):
                steps[k](imgs, caps, lens)
            steps[k].flush()
        rates = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, st in steps.items():
                decoder.bert_embedder = embedders[k]
                st(imgs, caps, lens)  # one batch in flight, as bench.py times the pipeline
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    st(imgs, caps, lens)
                torch.cuda.synchronize()
                rates[k].append(B * args.steps / (time.perf_counter() - t0))
                st.flush()
                torch.cuda.synchronize()
        res["config5_images_per_s"] = {k: summary(v) for k, v in rates.items()}
        res["config5_counts"] = {k: dict(st.counts) for k, st in steps.items()}
        for k, v in res["config5_images_per_s"].items():
            print(json.dumps({"arm": "config-5 step, " + k, "images_per_s": v}))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
