"""CPU: the fp64 restatement of the validation kernels' contracts (tests/eval_cases.py) is pinned to the
oracle's loss of a caption evaluated alone; capmi_eval_rows / capmi_eval_captions validate their arguments
before any launch; eval.py parses the reference's arguments and dispatches on the batch size."""
import ctypes
import types

import numpy as np
import pytest
import torch

import eval_cases as EC
import gen
from helpers import t


def test_restatement_is_the_oracle_loss_of_a_caption_alone():
    """rows_ref + captions_ref on the oracle's own logits and alphas give oracle.decoder_ref.attention_loss
    (CE mean over the caption's rows + ((1 - sum_t alpha)^2).mean()): both fp64, so only rounding separates them."""
    A, D, M, V, seed = 32, 32, 16, 50, 5
    p = {k: t(v) for k, v in gen.decoder_params(seed, A, D, M, V).items()}
    for L in (3, 6):
        cap = t(gen.captions(seed + L, 1, L, V))[0]
        feats = t(gen.encoder_features(seed + L, 1))
        o = EC.oracle_caption(p, feats, cap)
        T = L - 1
        assert o["decode_length"] == T and o["logits"].shape == (T, V)
        loss, pred, rank = EC.rows_ref(o["logits"][None], cap.view(1, -1).numpy(), [T])
        c = EC.captions_ref(loss, rank, o["alphas"][None], [T])
        assert abs(c["loss"][0] - o["loss"]) <= 1e-12 * max(1.0, abs(o["loss"]))
        assert c["top1"][0] == int((pred[0] == cap[1:].numpy()).sum())
        # the same caption inside a padded batch, at its own length: rows past it contribute nothing
        pad_logits = np.concatenate([o["logits"], np.full((2, V), 7.0)])[None]
        pad_alphas = np.concatenate([o["alphas"], np.full((2, o["alphas"].shape[1]), 0.3)])[None]
        pad_caps = np.concatenate([cap.numpy(), [0, 0]])[None]
        loss2, _, rank2 = EC.rows_ref(pad_logits, pad_caps, [T])
        c2 = EC.captions_ref(loss2, rank2, pad_alphas, [T])
        assert c2["loss"][0] == c["loss"][0] and c2["top5"][0] == c["top5"][0]


def test_restatement_tie_and_range_rules():
    x = np.array([[[0.0, 1.0, 1.0, 0.5, 0.5, 0.5]]], np.float32)
    for tgt, want_rank in ((1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (0, 5)):
        loss, pred, rank = EC.rows_ref(x, [[9, tgt]], None)
        assert pred[0, 0] == 1 and rank[0, 0] == want_rank and np.isfinite(loss[0, 0])
    for tgt in (-1, 6):
        loss, pred, rank = EC.rows_ref(x, [[9, tgt]], None)
        assert np.isposinf(loss[0, 0]) and rank[0, 0] == 6 and pred[0, 0] == 1
    loss, pred, rank = EC.rows_ref(x, [[9, 1]], [0])
    assert loss[0, 0] == 0 and pred[0, 0] == -1 and rank[0, 0] == -1
    c = EC.captions_ref(np.ones((2, 3)), np.array([[0, 4, 5], [0, 0, 0]]), np.full((2, 3, 2), 0.25), [9, -4])
    assert c["ce"].tolist() == [1.0, 0.0] and c["top1"].tolist() == [1, 0] and c["top5"].tolist() == [2, 0]
    assert c["reg"].tolist() == [0.0625, 0.0]


def test_constructed_cases_hold_the_ties_they_claim():
    for (B, T, V), pats in (((3, 3, 1027), EC.SCALAR_PATTERNS), ((1, 2, 8100), EC.VEC_PATTERNS)):
        x, caps = EC.constructed(B, T, V, 1)
        assert np.all(x * 4 == np.round(x * 4))  # the 1/4 grid: equalities are exact
        for r in range(B * T):
            row = x[r // T, r % T]
            assert sorted(np.flatnonzero(row == row.max()).tolist()) == sorted(pats[r % 4]) and len(pats[r % 4]) >= 2
            if r % 2 == 1:
                tgt = caps[r // T, r % T + 1]
                same = np.flatnonzero(row == row[tgt])
                assert same.min() < tgt < same.max() and row[tgt] == 0.5
    assert (1, 2, 8100) in EC.ROW_SHAPES and {s[2] for s in EC.ROW_SHAPES} >= {1, 50, 257, 1027, 8100}


def _lib():
    import capmi
    return capmi.lib


def test_eval_entry_points_reject_bad_arguments():
    """CAPMI_EINVAL (1001) before any launch: runs without a GPU."""
    lib = _lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p).value
    rows = [q, q, 2, 3, 4, 8, None, q, q, None, None]  # logits caps B T L V lens loss_rows pred rank stream
    for hole in (0, 1, 7, 8):
        a = list(rows)
        a[hole] = None
        assert lib.capmi_eval_rows(*a) == 1001, hole
    for pos, bad in ((2, 0), (2, -1), (3, 0), (5, 0), (5, -3), (4, 3), (4, 2)):  # B, T, V <= 0; L <= T
        a = list(rows)
        a[pos] = bad
        assert lib.capmi_eval_rows(*a) == 1001, (pos, bad)
    # loss_rows rank alphas lens B T P alpha_c cap_ce cap_reg cap_loss cap_top1 cap_top5 stream
    cap = [q, q, q, None, 2, 3, 4, 1.0, q, q, q, q, q, None]
    for hole in (0, 1, 2, 8, 9, 10, 11, 12):
        a = list(cap)
        a[hole] = None
        assert lib.capmi_eval_captions(*a) == 1001, hole
    for pos in (4, 5, 6):
        for bad in (0, -2):
            a = list(cap)
            a[pos] = bad
            assert lib.capmi_eval_captions(*a) == 1001, (pos, bad)


def test_new_entry_points_are_declared_and_bound_without_an_abi_bump():
    import capmi
    from capmi import kernels as K
    assert {"capmi_eval_rows", "capmi_eval_captions"} <= set(capmi.EXPORTS)
    assert capmi.ABI_VERSION == 27 == capmi.lib.capmi_abi_version()
    assert callable(K.eval_rows) and callable(K.eval_captions)
    with pytest.raises(ValueError):  # host tensors are refused: there is no CPU fallback
        K.eval_rows(torch.zeros(1, 1, 4), torch.zeros(1, 2, dtype=torch.int64), 1, 1, 2, 4, None,
                    torch.zeros(1), torch.zeros(1, dtype=torch.int32))


def test_stale_library_is_an_import_error(monkeypatch):
    """A libcapmi.so built before an entry point was added (same ABI number) asks for a rebuild."""
    from capmi import _lib
    monkeypatch.setitem(_lib._SIGS, "capmi_not_built_yet", [])
    with pytest.raises(ImportError, match="rebuild"):
        _lib._load()


def test_get_eval_score_is_still_unavailable():
    """models.attention.evaluate falls back to references / hypotheses on this (tests/test_gpu_beam.py)."""
    from metric import get_eval_score
    with pytest.raises(NotImplementedError):
        get_eval_score([[[1, 2]]], [[1, 2]])


# ---------------------------------------------------------------------------------------------------
# eval.py
# ---------------------------------------------------------------------------------------------------
def test_eval_cli_arguments():
    import eval as E
    a = E.parse_args(["basic_att_3.pth.tar", "--model_type", "attention"])
    assert (a.checkpoint, a.model_type, a.max_caption_length, a.print_freq) == ("basic_att_3.pth.tar", "attention", -1, 1)
    assert a.batch_size == 1 and a.synthetic_size == 0 and a.vocab_size == 8100 and a.synthetic_len == 25
    a = E.parse_args(["c.pth.tar", "--model_type", "attention", "--batch_size", "64", "--synthetic_size", "12",
                      "--vocab_size", "50", "--synthetic_len", "8", "--print_freq", "5", "--max_caption_length", "30"])
    assert (a.batch_size, a.synthetic_size, a.vocab_size, a.synthetic_len, a.print_freq) == (64, 12, 50, 8, 5)
    assert a.max_caption_length == 30
    with pytest.raises(SystemExit):
        E.parse_args(["c.pth.tar", "--model_type", "transformer"])
    with pytest.raises(SystemExit):
        E.parse_args(["c.pth.tar", "--model_type", "attention", "--batch_size", "0"])


@pytest.mark.parametrize("batch_size", [1, 4])
def test_eval_cli_dispatch(monkeypatch, tmp_path, batch_size):
    """Batch size 1 runs the reference loop (evaluate), larger the batched pass; the metrics land in
    <eval_data>/<checkpoint stem>.json. Checkpoint loading and both evaluators are stubbed."""
    import json
    import eval as E
    import models.attention as MA
    import models.baseline as MB
    calls = []
    mod = types.SimpleNamespace(state_dict=lambda: {}, to=lambda dev: mod)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(E, "load_checkpoint", lambda device, args, **kw: {
        "epoch": 0, "encoder": mod, "decoder": mod, "encoder_optimizer": None, "decoder_optimizer": None,
        "metrics": {}})

    def fake_evaluate(device, args, encoder, decoder, val_loader=None):
        calls.append(("evaluate", val_loader))
        return {"losses": [1.0]}

    def fake_batched(device, args, encoder, decoder, dataset=None, batch_size=64):
        calls.append(("evaluate_batched", dataset, batch_size))
        return {"losses": [1.0, 2.0], "Bleu_1": 0.5}

    monkeypatch.setattr(MA, "evaluate", fake_evaluate)
    monkeypatch.setattr(MA, "evaluate_batched", fake_batched)
    monkeypatch.setattr(MB, "evaluate", lambda device, args, encoder, decoder: calls.append(("baseline",)) or {"b": 1})
    out = E.main(["run7_2.pth.tar", "--model_type", "attention", "--batch_size", str(batch_size)])
    assert len(calls) == 1
    if batch_size == 1:
        assert calls[0] == ("evaluate", None) and out == {"losses": [1.0]}
    else:
        assert calls[0] == ("evaluate_batched", None, 4) and out["Bleu_1"] == 0.5
    with open(tmp_path / "eval_data" / "run7_2.json") as f:
        assert json.load(f) == out
    del calls[:]
    E.main(["run7_2.pth.tar", "--model_type", "baseline", "--batch_size", str(batch_size)])
    assert calls == [("baseline",)]
