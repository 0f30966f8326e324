"""GPU: the real BERT feature producer (capmi/bert.py, csrc/bert.hip).

Kernels alone and the whole embedder against fp64 torch (tests/bert_cases.py, itself pinned to
transformers.BertModel in test_bert_cpu.py). Tolerances: these are fp32 elementwise / reduction kernels that
sum in another order than torch's CPU kernels, so each check measures the fp32 CPU restatement's own max error
against fp64 on the same inputs and allows 4x that (DESIGN section 5's rule for a different summation order);
the bf16 embedder must be within 2x the error of the restatement whose GEMM operands are rounded to bf16
(the rule of test_gpu_bench_paths.py for the bf16 encoder). Both numbers are in every assertion message."""
import json
import math
import os

import pytest
import torch

import bert_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def within(got, ref64, base, factor, what):
    """max|got - ref64| <= factor * max|base - ref64| (base: the CPU restatement that sets the error scale)."""
    e_gpu = float((got.detach().double().cpu() - ref64).abs().max())
    e_cpu = float((base.detach().double().cpu() - ref64).abs().max())
    print(f"{what}: GPU max error {e_gpu:.4e}, CPU restatement max error {e_cpu:.4e}, allowed {factor} x")
    assert math.isfinite(e_gpu) and e_gpu <= factor * e_cpu, \
        f"{what}: GPU max error {e_gpu:.4e} > {factor} x the CPU restatement's {e_cpu:.4e}"


def rnd(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


# ------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("hidden", [128, 768])
def test_embed_ln(rows, hidden):
    from capmi import kernels as K
    V, P, eps = 37, 70, 1e-12
    we, pe, te = rnd(V, hidden, seed=1), rnd(P, hidden, seed=2, std=0.3), rnd(2, hidden, seed=3, std=0.3)
    g, b = 1 + rnd(hidden, seed=4, std=0.1), rnd(hidden, seed=5, std=0.1)
    gen = torch.Generator().manual_seed(6)
    ids = torch.randint(0, V, (rows,), generator=gen)
    pos = torch.randint(0, P, (rows,), generator=gen)
    ids[0], pos[0] = V - 1, P - 1  # the last table rows

    def ref(dt):
        return BC.layer_norm_ref(we.to(dt)[ids] + pe.to(dt)[pos] + te.to(dt)[0], g.to(dt), b.to(dt), eps)
    out = torch.full((rows + 1, hidden), float("nan"), device=DEV)
    K.bert_embed_ln(we.to(DEV), pe.to(DEV), te.to(DEV), ids.to(DEV, torch.int32), pos.to(DEV, torch.int32), rows,
                    g.to(DEV), b.to(DEV), eps, out)
    torch.cuda.synchronize()
    assert bool(out[rows].isnan().all())  # nothing past the last row
    within(out[:rows], ref(F64), ref(torch.float32), 4, f"embed_ln rows {rows} hidden {hidden}")


def _attention_case(lens, heads, qkv, what):
    from capmi import kernels as K
    H = heads * 64
    rows = sum(lens)
    off = [0]
    for n in lens:
        off.append(off[-1] + n)

    def ref(dt):
        z = qkv.to(dt)
        return torch.cat([BC.attention_ref(z[a:b, :H], z[a:b, H:2 * H], z[a:b, 2 * H:], heads)
                          for a, b in zip(off[:-1], off[1:])])
    out = torch.full((rows + 1, H), float("nan"), device=DEV)
    K.bert_attention(qkv.to(DEV), torch.tensor(off, dtype=torch.int32, device=DEV), len(lens), rows, max(lens), heads,
                     64, out)
    torch.cuda.synchronize()
    assert bool(out[rows].isnan().all())
    assert not bool(out[:rows].isnan().any())
    within(out[:rows], ref(F64), ref(torch.float32), 4, what)


def test_attention_ragged_lengths():
    lens = [1, 2, 63, 64, 65, 130]  # below, at and above the 64-query / 64-key block, and three key blocks
    _attention_case(lens, 2, rnd(sum(lens), 3 * 128, seed=11), "attention ragged")


def test_attention_longest_sequence():
    _attention_case([512], 2, rnd(512, 3 * 128, seed=12), "attention n=512")


@pytest.mark.parametrize("span", [80.0, 200.0])
def test_attention_wide_scores(span):
    """Rows whose scores run from -span to +span, to catch an unsafe softmax: +-80 (exp of the raw scores
    reaches 5e34 and 2e-35, the edge of fp32's normal range) and +-200 (exp of the raw score is inf)."""
    n, heads, H = 48, 2, 128
    qkv = rnd(n, 3 * H, seed=13)
    qkv[:, :H] = 1.0  # every q = ones: score_j = sum(k_j) / 8
    qkv[:, H:2 * H] = torch.linspace(-span / 8, span / 8, n).view(n, 1)  # 64 k / 8 = -span .. span
    _attention_case([n], heads, qkv, f"attention scores +-{span:g}")


@pytest.mark.parametrize("cols", [256, 3072])
def test_bias_gelu(cols):
    from capmi import kernels as K
    rows = 5
    x, bias = rnd(rows, cols, seed=21, std=2.0), rnd(cols, seed=22, std=0.5)
    buf = torch.full((rows + 1, cols), float("nan"), device=DEV)
    buf[:rows] = x.to(DEV)
    K.bias_gelu(buf, bias.to(DEV), rows, cols)
    torch.cuda.synchronize()
    assert bool(buf[rows].isnan().all())
    within(buf[:rows], BC.gelu_ref(x.double() + bias.double()), BC.gelu_ref(x + bias), 4, f"bias_gelu cols {cols}")


@pytest.mark.parametrize("hidden", [128, 768])
def test_add_ln(hidden):
    from capmi import kernels as K
    rows, eps = 67, 1e-12
    x, res, bias = rnd(rows, hidden, seed=31), rnd(rows, hidden, seed=32), rnd(hidden, seed=33, std=0.3)
    g, b = 1 + rnd(hidden, seed=34, std=0.1), rnd(hidden, seed=35, std=0.1)

    def ref(dt, with_bias):
        s = x.to(dt) + (bias.to(dt) if with_bias else 0) + res.to(dt)
        return BC.layer_norm_ref(s, g.to(dt), b.to(dt), eps)
    for with_bias in (True, False):
        out = torch.full((rows + 1, hidden), float("nan"), device=DEV)
        K.add_ln(x.to(DEV), bias.to(DEV) if with_bias else None, res.to(DEV), rows, hidden, g.to(DEV), b.to(DEV), eps,
                 out)
        torch.cuda.synchronize()
        assert bool(out[rows].isnan().all())
        within(out[:rows], ref(F64, with_bias), ref(torch.float32, with_bias), 4,
               f"add_ln hidden {hidden} bias {with_bias}")


def test_segment_sum_rows():
    from capmi import kernels as K
    hidden, seg = 128, [0, 1, 4, 11, 11]  # segments of 1, 3 and 7 pieces, and an empty one
    x = rnd(11, hidden, seed=41)
    out = torch.full((len(seg) - 1 + 2, hidden), float("nan"), device=DEV)  # two NaN sentinel rows after
    K.segment_sum_rows(x.to(DEV), torch.tensor(seg, dtype=torch.int32, device=DEV), len(seg) - 1, 11, hidden, out)
    torch.cuda.synchronize()
    assert bool(out[len(seg) - 1:].isnan().all()), "sentinel rows after the output were written"

    def ref(dt):
        return torch.stack([x.to(dt)[a:b].sum(0) for a, b in zip(seg[:-1], seg[1:])])
    assert torch.equal(out[0].cpu(), x[0]) and float(out[3].abs().max()) == 0.0
    within(out[:len(seg) - 1], ref(F64), ref(torch.float32), 4, "segment_sum_rows")


# ------------------------------------------------------------------------------------------ whole embedder
def _tokens(vocab, B, L, seed):
    """Captions with pads, multi-piece words ('unbelievable', 'it's', 'w12') and an [UNK] word ('zebra')."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, len(vocab) - 3, (B, L), generator=g)
    tok[:, 0] = vocab("<start>")
    tok[0, 1], tok[0, 2], tok[1, 1], tok[1, 2] = vocab("unbelievable"), vocab("zebra"), vocab("it's"), vocab("w12")
    tok[1, L - 2:] = vocab("<pad>")
    tok[1, L - 3] = vocab("<end>")
    tok[2, L - 1] = vocab("<end>")
    return tok


class Case:
    def __init__(self, tmp, config, B, L, layers):
        from capmi.text import WordPieceTokenizer
        self.vocab = BC.caption_vocab()
        self.weights = BC.make_weights(config, 77, BC.write_vocab(tmp))
        self.tokenizer = WordPieceTokenizer(self.weights.vocab_file)
        self.tokens = _tokens(self.vocab, B, L, 5)
        self.ref = {}
        for layer in layers:
            r = lambda dt, ro=False: BC.word_features_ref(self.weights, self.tokenizer, self.vocab, self.tokens,  # noqa: E731
                                                          layer, dt, ro)
            self.ref[layer] = {"f64": r(F64), "f32": r(torch.float32), "bf16": r(F64, True)}

    def check(self, precision, layer):
        from capmi.bert import BertEmbedder
        emb = BertEmbedder(self.vocab, self.weights, DEV, precision=precision, layer=layer)
        out = emb(self.tokens.to(DEV))
        torch.cuda.synchronize()
        B, L = self.tokens.shape
        assert tuple(out.shape) == (B, L + 1, self.weights.config["hidden_size"]) and out.dtype == torch.float32
        assert len(set(torch.diff(torch.from_numpy(emb.last_layout["seq_off"])).tolist())) > 1  # ragged
        ref = self.ref[layer]
        if precision == "bf16":
            within(out, ref["f64"], ref["bf16"], 2, f"embedder bf16 layer {layer}")
        else:
            within(out, ref["f64"], ref["f32"], 4, f"embedder {precision} layer {layer}")
        return out


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("small"), BC.SMALL, 5, 7, (0, 1))


@pytest.fixture(scope="module")
def base1(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("base1"), BC.BASE_1LAYER, 3, 6, (0,))


@pytest.mark.parametrize("precision", ["fp32-x3", "fp32", "bf16"])
def test_embedder_small_config(small, precision):
    small.check(precision, 1)


@pytest.mark.parametrize("precision", ["fp32-x3", "bf16"])
def test_embedder_production_geometry_one_layer(base1, precision):
    base1.check(precision, 0)


def test_layer_selects_the_layer(small):
    o0, o1 = small.check("fp32", 0), small.check("fp32", 1)
    assert float((o0 - o1).abs().max()) > 1e-2


def test_caption_longer_than_position_table_raises(small):
    from capmi.bert import BertEmbedder
    emb = BertEmbedder(small.vocab, small.weights, DEV, precision="fp32", layer=0)
    tok = torch.full((1, 40), small.vocab("unbelievable"))  # 1 + 40 * 3 pieces > 64 positions
    with pytest.raises(ValueError, match="position"):
        emb(tok)


# ------------------------------------------------------------------------------------------ plumbing
def test_fused_step_with_real_embedder_equals_precomputed_features(small):
    """capmi.decoder_fn.fused_loss_and_grads on a tiny use_bert decoder: the real embedder and a stub returning
    the same feature tensor give bit-equal loss, predictions, alphas and gradients."""
    import gen
    from helpers import t
    from capmi import decoder_fn as DF
    from capmi.bert import BertEmbedder
    from models.attention import AttentionDecoder, AttentionDecoderParams
    torch.manual_seed(9)
    prm = AttentionDecoderParams()
    prm.attention_dim, prm.decoder_dim, prm.embed_size, prm.dropout = 32, 32, 128, 0.0
    prm.vocab, prm.use_bert = small.vocab, True
    dec = AttentionDecoder(DEV, prm).to(DEV).train()
    B, L = small.tokens.shape
    enc, caps = t(gen.encoder_features(9, B), DEV), small.tokens.to(DEV)
    emb = BertEmbedder(small.vocab, small.weights, DEV, precision="fp32", layer=1)
    feats = emb(caps).clone()
    named = dict(dec.named_parameters())
    res = []
    for embedder in (emb, lambda c: feats):
        dec.bert_embedder = embedder
        grads = {n: torch.zeros_like(q) for n, q in named.items() if q.requires_grad}
        loss, preds, alphas = DF.fused_loss_and_grads(dec, enc, caps, [L] * B, 1.0, grads)
        torch.cuda.synchronize()
        res.append((loss.clone(), preds.clone(), alphas.clone(), {n: g.clone() for n, g in grads.items()}))
    (l0, p0, a0, g0), (l1, p1, a1, g1) = res
    assert math.isfinite(float(l0)) and torch.equal(l0, l1) and torch.equal(p0, p1) and torch.equal(a0, a1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert float(g0["fc.weight"].abs().max()) > 0


def test_train_with_bert_path(tmp_path, monkeypatch):
    """models.attention.train with --use_bert True --bert_path <local checkpoint> runs (two steps of 8 over a
    16-item synthetic set) with finite, sane losses, in the graph launch mode train() uses and eagerly, with the
    same losses. Without the feature the first step raises the bert_embedder RuntimeError."""
    import types
    import checkpoint as C
    from models import attention as A
    from capmi.bert import BertEmbedder
    monkeypatch.setattr(C, "CHECKPOINTS_DIR", str(tmp_path / "ck"))
    bert_dir = tmp_path / "bert"
    bert_dir.mkdir()
    V = 50
    torch.save(BC.random_tensors(BC.SMALL, len(BC.VOCAB_PIECES), 3), bert_dir / "pytorch_model.bin")
    with open(bert_dir / "config.json", "w") as f:
        json.dump(dict(BC.SMALL, vocab_size=len(BC.VOCAB_PIECES)), f)
    BC.write_vocab(bert_dir)
    losses = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("CAPMI_TRAIN_GRAPH", mode)
        torch.manual_seed(0)
        args = types.SimpleNamespace(
            model_name=f"bert{mode}", model="attention", attention_dim=32, decoder_dim=32, decoder_dropout=0.5,
            embed_size=128, epochs=1, batch_size=8, workers=0, encoder_lr=1e-4, decoder_lr=1e-4, grad_clip=5.0,
            alpha_c=1.0, fine_tune_encoder=False, fine_tune_embedding=False, checkpoint=None, print_freq=1,
            use_glove=False, max_caption_length=-1, use_bert=True, bert_path=str(bert_dir), synthetic=True,
            synthetic_size=16, synthetic_len=9, vocab_size=V, trusted_checkpoint=False)
        A.train(torch.device(DEV), args)
        step = A.train.last_step
        assert isinstance(step.decoder.bert_embedder, BertEmbedder)
        assert step.pipe_graph == (mode == "1")
        ck = torch.load(tmp_path / "ck" / f"bert{mode}_0.pth.tar", weights_only=True)
        assert not any("bert" in k for k in ck["decoder"])  # not a submodule: checkpoints keep their keys
        losses[mode] = ck["metrics"]["epoch_losses"][0]
    assert len(losses["1"]) == 2 and all(math.isfinite(x) for x in losses["1"])
    # a fresh decoder: CE about ln V plus the attention regulariser (at most 1): far below 3 ln V
    assert all(0.0 < x < 3 * math.log(V) for x in losses["1"]), losses
    assert losses["1"] == losses["0"], losses
    assert A.train.last_step.counts["replay"] == 0
    assert os.path.exists(tmp_path / "ck" / "bert1_0.pth.tar")
