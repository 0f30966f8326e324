"""CPU: the pieces of the real-BERT feature producer that need no GPU -- the WordPiece tokenizer, the
torch restatement the GPU tests compare against (pinned to transformers.BertModel where it is installed),
the per-vocabulary piece table, the host-side ragged batch layout, the checkpoint loader, the argument
validation of the new exports, and the unchanged no-path behaviour."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import bert_cases as BC

TOKENIZER_CASES = [
    ("<pad>", ["<", "pad", ">"]),
    ("<start> a dog <end>", ["<", "start", ">", "a", "dog", "<", "end", ">"]),
    ("<unk>", ["<", "unk", ">"]),
    ("unbelievable", ["un", "##believ", "##able"]),
    ("playing cats", ["play", "##ing", "cat", "##s"]),
    ("it's", ["it", "'", "s"]),
    ("zebra", ["[UNK]"]),
    ("The DOG", ["the", "dog"]),
    ("café", ["cafe"]),
    ("w12 w907", ["w", "##1", "##2", "w", "##9", "##0", "##7"]),
    ("[CLS] a dog.", ["[CLS]", "a", "dog", "."]),
    ("a" * 101 + " cat", ["[UNK]", "cat"]),
]


@pytest.fixture(scope="module")
def vocab_file(tmp_path_factory):
    return BC.write_vocab(tmp_path_factory.mktemp("wp"))


@pytest.fixture(scope="module")
def tokenizer(vocab_file):
    from capmi.text import WordPieceTokenizer
    return WordPieceTokenizer(vocab_file)


@pytest.mark.parametrize("text,want", TOKENIZER_CASES)
def test_wordpiece_fixed_cases(tokenizer, text, want):
    assert tokenizer.tokenize(text) == want
    assert tokenizer.convert_tokens_to_ids(want) == [BC.VOCAB_PIECES.index(p) for p in want]


def test_wordpiece_matches_transformers(tokenizer, vocab_file):
    transformers = pytest.importorskip("transformers")
    hf = transformers.BertTokenizer(vocab_file)
    for text, _ in TOKENIZER_CASES:
        assert tokenizer.tokenize(text) == hf.tokenize(text), text


def test_restatement_matches_transformers(vocab_file):
    """bert_forward_ref in fp64 == transformers.BertModel(...).double() hidden_states[layer + 1] to 1e-10."""
    transformers = pytest.importorskip("transformers")
    cfg = dict(BC.SMALL)
    torch.manual_seed(3)
    model = transformers.BertModel(transformers.BertConfig(vocab_size=len(BC.VOCAB_PIECES), **cfg)).double().eval()
    from capmi.bert import BertWeights
    w = BertWeights(model.state_dict(), cfg, vocab_file)
    ids = [2, 5, 8, 6, 22, 24, 29, 30, 31, 1, 43]
    with torch.no_grad():
        hs = model(input_ids=torch.tensor([ids]), output_hidden_states=True).hidden_states
    for layer in (0, 1):
        # (the model was initialised in fp32 and widened: BertWeights' fp32 copy of it is exact)
        got = BC.bert_forward_ref(w, ids, layer, torch.float64)
        err = float((got - hs[layer + 1][0]).abs().max())
        assert err <= 1e-10, (layer, err)


def test_piece_table_concatenates(tokenizer):
    from capmi.text import word_pieces
    v = BC.caption_vocab()
    off, ids = word_pieces(v, tokenizer)
    assert off.dtype == np.int64 and ids.dtype == np.int32 and len(off) == len(v) + 1 and off[-1] == len(ids)
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        cap = torch.randint(0, len(v), (9,), generator=g).tolist()
        joined = tokenizer.convert_tokens_to_ids(tokenizer.tokenize(" ".join(v.i2w[i] for i in cap)))
        assert [int(p) for i in cap for p in ids[off[i]:off[i + 1]]] == joined
    pad = v("<pad>")
    assert tokenizer.vocab["<"] == ids[off[pad]] and off[pad + 1] - off[pad] == 3  # '<', 'pad', '>'
    assert [int(p) for p in ids[off[v("zebra")]:off[v("zebra") + 1]]] == [tokenizer.vocab["[UNK]"]]


def test_batch_layout_matches_loop(tokenizer):
    from capmi.bert import batch_layout
    from capmi.text import word_pieces
    v = BC.caption_vocab()
    off, ids = word_pieces(v, tokenizer)
    cls_id = tokenizer.vocab["[CLS]"]
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, len(v), (6, 8), generator=g)
    tokens[2, 4:] = v("<pad>")  # a padded caption: pads are words
    lay = batch_layout(tokens.numpy(), off, ids, cls_id)
    want_ids, want_pos, seq_off, seg_off = [], [], [0], [0]
    for cap in tokens.tolist():
        seq = [cls_id]
        seg_off.append(seg_off[-1] + 1)
        for wd in cap:
            pieces = [int(p) for p in ids[off[wd]:off[wd + 1]]]
            seq += pieces
            seg_off.append(seg_off[-1] + len(pieces))
        want_ids += seq
        want_pos += list(range(len(seq)))
        seq_off.append(seq_off[-1] + len(seq))
    assert lay["ids"].tolist() == want_ids and lay["pos"].tolist() == want_pos
    assert lay["seq_off"].tolist() == seq_off and lay["seg_off"].tolist() == seg_off
    assert lay["rows"] == len(want_ids) and lay["max_len"] == max(np.diff(seq_off))
    assert len(set(np.diff(seq_off).tolist())) > 1  # the batch is ragged
    assert all(a.dtype == np.int32 for a in (lay["ids"], lay["pos"], lay["seq_off"], lay["seg_off"]))
    with pytest.raises(IndexError):
        batch_layout(np.array([[len(v)]]), off, ids, cls_id)


def _save(dirname, tensors, cfg, cfg_name="config.json"):
    d = str(dirname)
    torch.save(tensors, os.path.join(d, "pytorch_model.bin"))
    with open(os.path.join(d, cfg_name), "w") as f:
        json.dump(cfg, f)
    BC.write_vocab(d)
    return d


def test_loader_key_forms(tmp_path):
    from capmi.bert import BertWeights
    cfg = dict(BC.SMALL)
    base = BC.random_tensors(cfg, len(BC.VOCAB_PIECES), 5)
    forms = {
        "hf": dict(base),
        "gamma_beta": {k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta"): v
                       for k, v in base.items()},
        "bert": {"bert." + k: v for k, v in base.items()},
        "bert_model": {"bert_model." + k: v for k, v in base.items()},
    }
    forms["bert"]["bert.pooler.dense.weight"] = torch.zeros(4, 4)  # pooler and heads are ignored
    forms["bert"]["cls.predictions.bias"] = torch.zeros(4)
    forms["bert_model"]["fc.weight"] = torch.zeros(2, 2)  # a decoder state_dict carries its own keys too
    loaded = {}
    for name, sd in forms.items():
        d = tmp_path / name
        d.mkdir()
        loaded[name] = BertWeights.load(_save(d, sd, cfg, "bert_config.json" if name == "bert" else "config.json"))
        assert loaded[name].vocab_file == os.path.join(str(d), "vocab.txt")
    for name, w in loaded.items():
        assert set(w.tensors) == set(base), name
        for k, v in base.items():
            assert torch.equal(w.tensors[k], v), (name, k)
    # the weights file itself is accepted too
    assert set(BertWeights.load(os.path.join(str(tmp_path / "hf"), "pytorch_model.bin")).tensors) == set(base)


def test_loader_missing_key_is_named(tmp_path):
    from capmi.bert import BertWeights
    cfg = dict(BC.SMALL)
    sd = BC.random_tensors(cfg, len(BC.VOCAB_PIECES), 5)
    del sd["encoder.layer.1.output.dense.bias"]
    del sd["embeddings.LayerNorm.weight"]
    with pytest.raises(KeyError) as e:
        BertWeights.load(_save(tmp_path, sd, cfg))
    assert "encoder.layer.1.output.dense.bias" in str(e.value) and "embeddings.LayerNorm.weight" in str(e.value)


def test_loader_never_fetches_by_name(monkeypatch, tmp_path):
    import socket
    from capmi.bert import BertWeights

    def no_network(*a, **k):
        raise AssertionError("network attempt")
    monkeypatch.setattr(socket, "socket", no_network)
    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket, "getaddrinfo", no_network)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="never fetched"):
        BertWeights.load("bert-base-uncased")


def test_new_exports_validate_without_a_gpu():
    import capmi
    from capmi._lib import lib
    assert capmi.ABI_VERSION == 27 and lib.capmi_abi_version() == 27
    assert lib.capmi_bert_embed_ln(None, None, None, None, None, 4, 128, 10, 10, None, None, 1e-12, None, None) == 1001
    assert lib.capmi_add_ln(None, None, None, 4, 128, None, None, 1e-12, None, None) == 1001
    assert lib.capmi_bias_gelu(None, None, 4, 128, 128, None) == 1001
    assert lib.capmi_bert_attention(None, None, 1, 4, 4, 2, 64, None, 128, None) == 1001
    assert lib.capmi_segment_sum_rows(None, None, 2, 4, 128, None, None) == 1001
    p = ctypes.c_void_p(4096)  # a 16-B aligned stand-in: validation never dereferences it
    assert lib.capmi_bert_attention(p, p, 1, 4, 4, 2, 32, p, 64, None) == 1003  # head dim 32: CAPMI_ERANGE
    assert lib.capmi_bert_attention(p, p, 1, 600, 513, 2, 64, p, 128, None) == 1003  # sequences longer than 512
    assert lib.capmi_bert_attention(p, p, 0, 4, 4, 2, 64, p, 128, None) == 1001
    assert lib.capmi_add_ln(p, None, p, 4, 130, p, p, 1e-12, p, None) == 1001  # hidden % 4
    assert lib.capmi_bias_gelu(p, None, 4, 128, 64, None) == 1001  # ld < cols
    assert lib.capmi_segment_sum_rows(p, p, 0, 4, 128, p, None) == 1001
    assert lib.capmi_bert_embed_ln(p, p, p, p, p, 0, 128, 10, 10, p, p, 1e-12, p, None) == 1001


def test_use_bert_without_a_path_still_raises():
    from models.attention import AttentionDecoder, AttentionDecoderParams
    from pathconf import PathConfig
    from train import parse_args
    from vocabulary import synthetic_vocab
    args = parse_args(["x", "--model", "attention", "--use_bert", "True", "--embed_size", "768"])
    assert args.bert_path is None
    assert parse_args(["x", "--bert_path", "some/dir"]).bert_path == "some/dir"
    assert hasattr(PathConfig, "bert_dir")
    p = AttentionDecoderParams()
    p.attention_dim, p.decoder_dim, p.embed_size, p.use_bert = 32, 32, 768, True
    p.vocab = synthetic_vocab(50)
    d = AttentionDecoder(torch.device("cpu"), p)
    assert d.bert_embedder is None
    with pytest.raises(RuntimeError, match="needs decoder.bert_embedder"):
        d.bert_embeddings(torch.zeros(2, 5, dtype=torch.long))
    assert not any("bert" in k for k in d.state_dict())
