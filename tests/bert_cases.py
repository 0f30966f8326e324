"""Shared cases of the BERT feature tests (not a test file): a small WordPiece vocabulary, a seeded
random-weights generator, and the plain-torch restatement of the BERT encoder forward that the reference
runs one caption at a time (models/attention.py:166-215), with its piece -> word pooling rule."""
import math
import os

import torch

VOCAB_PIECES = [
    "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]",
    "<", ">", "pad", "start", "end", "unk", "w",
    "##0", "##1", "##2", "##3", "##4", "##5", "##6", "##7", "##8", "##9",
    "a", "the", "dog", "cat", "play", "##ing", "##s", "un", "##believ", "##able", "it", "s", "cafe",
    "on", "sit", "##ting", "table", "0", "1", "2",
    "'", ".", ",", "!", "-", "#",
]
VOCAB_TXT = "\n".join(VOCAB_PIECES) + "\n"

SMALL = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
             max_position_embeddings=64, type_vocab_size=2, layer_norm_eps=1e-12)
BASE_1LAYER = dict(hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=3072,
                   max_position_embeddings=64, type_vocab_size=2, layer_norm_eps=1e-12)


def write_vocab(dirname, text=VOCAB_TXT):
    path = os.path.join(str(dirname), "vocab.txt")
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    return path


def random_tensors(config, vocab_size, seed):
    """HF-named fp32 tensors of a BERT encoder: weights N(0, 0.05^2) (attention scores and GELU inputs of
    order one), LayerNorm gains 1 +- 0.1, small biases."""
    g = torch.Generator().manual_seed(seed)
    H, I = config["hidden_size"], config["intermediate_size"]

    def n(*shape, std=0.05):
        return torch.randn(*shape, generator=g) * std

    t = {"embeddings.word_embeddings.weight": n(vocab_size, H, std=0.5),
         "embeddings.position_embeddings.weight": n(config["max_position_embeddings"], H, std=0.2),
         "embeddings.token_type_embeddings.weight": n(config["type_vocab_size"], H, std=0.2),
         "embeddings.LayerNorm.weight": 1 + n(H, std=0.1), "embeddings.LayerNorm.bias": n(H)}
    for i in range(config["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        for name, (o, k) in {"attention.self.query": (H, H), "attention.self.key": (H, H),
                             "attention.self.value": (H, H), "attention.output.dense": (H, H),
                             "intermediate.dense": (I, H), "output.dense": (H, I)}.items():
            t[p + name + ".weight"] = n(o, k, std=0.08 if "self" in name else 0.05)
            t[p + name + ".bias"] = n(o)
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            t[p + name + ".weight"] = 1 + n(H, std=0.1)
            t[p + name + ".bias"] = n(H)
    return t


def make_weights(config, seed, vocab_file, vocab_size=len(VOCAB_PIECES)):
    from capmi.bert import BertWeights
    return BertWeights(random_tensors(config, vocab_size, seed), config, vocab_file)


def layer_norm_ref(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu_ref(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention_ref(q, k, v, heads):
    """(n, H) each -> (n, H): per head softmax(q k^T / sqrt(d)) v."""
    n, H = q.shape
    d = H // heads
    qh, kh, vh = (z.view(n, heads, d).transpose(0, 1) for z in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(d), dim=-1)
    return (p @ vh).transpose(0, 1).reshape(n, H)


def bert_forward_ref(weights, piece_ids, layer, dtype, round_operands=False):
    """Hidden states after encoder layer ``layer`` (HF hidden_states[layer + 1]) of ONE sequence of piece ids
    (token_type 0, positions 0.., full attention), computed in ``dtype``. round_operands: both operands of every
    Linear GEMM are rounded to bf16 first (the CAPMI_GEMM_BF16 operand contract), everything else in ``dtype``."""
    cfg = weights.config
    T = {k: v.to(dtype) for k, v in weights.tensors.items()}
    eps, heads = cfg["layer_norm_eps"], cfg["num_attention_heads"]

    def rnd(z):
        return z.to(torch.float32).to(torch.bfloat16).to(dtype) if round_operands else z

    def linear(x, name):
        return rnd(x) @ rnd(T[name + ".weight"]).t() + T[name + ".bias"]

    ids = torch.as_tensor(piece_ids, dtype=torch.long)
    x = (T["embeddings.word_embeddings.weight"][ids] + T["embeddings.position_embeddings.weight"][:len(ids)]
         + T["embeddings.token_type_embeddings.weight"][0])
    x = layer_norm_ref(x, T["embeddings.LayerNorm.weight"], T["embeddings.LayerNorm.bias"], eps)
    for i in range(layer + 1):
        p = f"encoder.layer.{i}."
        q, k, v = (linear(x, p + f"attention.self.{n}") for n in ("query", "key", "value"))
        a = linear(attention_ref(q, k, v, heads), p + "attention.output.dense")
        x = layer_norm_ref(a + x, T[p + "attention.output.LayerNorm.weight"], T[p + "attention.output.LayerNorm.bias"],
                           eps)
        f = linear(gelu_ref(linear(x, p + "intermediate.dense")), p + "output.dense")
        x = layer_norm_ref(f + x, T[p + "output.LayerNorm.weight"], T[p + "output.LayerNorm.bias"], eps)
    return x


def word_features_ref(weights, tokenizer, vocab, tokens, layer, dtype, round_operands=False):
    """(B, L) caption tokens -> (B, L+1, hidden): one caption at a time, row 0 = [CLS], row 1+i = the sum of the
    layer outputs of word i's pieces (pads are ordinary words)."""
    out = []
    cls_id = tokenizer.vocab["[CLS]"]
    for cap in torch.as_tensor(tokens).tolist():
        words = [tokenizer.encode_word(vocab.i2w[w]) for w in cap]
        ids = [cls_id] + [p for w in words for p in w]
        h = bert_forward_ref(weights, ids, layer, dtype, round_operands)
        rows, at = [h[0]], 1
        for w in words:
            rows.append(h[at:at + len(w)].sum(0) if w else torch.zeros_like(h[0]))
            at += len(w)
        out.append(torch.stack(rows))
    return torch.stack(out)


def caption_vocab():
    """A caption Vocabulary in the reference layout whose words exercise every pooling case: single pieces,
    ## chains, punctuation inside a word, an accent, an unknown word."""
    from vocabulary import END_TOKEN, PAD_TOKEN, START_TOKEN, UNK_TOKEN, Vocabulary
    v = Vocabulary()
    v.add_word(PAD_TOKEN)
    for w in ("a", "the", "dog", "cats", "playing", "unbelievable", "it's", "café", "zebra", "w12", "sitting",
              "table", ".", "on"):
        v.add_word(w)
    for tok in (START_TOKEN, END_TOKEN, UNK_TOKEN):
        v.add_word(tok)
    return v
