"""CPU: models.baseline.evaluate at batch 1 (plain nn.LSTM) against the fp64 oracle of every caption alone;
eval.py rebuilds the baseline modules from a state_dict checkpoint; the new entry points are declared, exported
and validate their arguments before any launch; the CPU beam helper at k = 1 is a greedy loop."""
import ctypes
import types

import numpy as np
import pytest
import torch

import baseline_cases as BC
import eval_cases as EC
import gen

E2E_SEED = 75


def _close(got, want):
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


def test_evaluate_batch_1_matches_the_fp64_oracle():
    from models.baseline import evaluate
    c = BC.E2E
    items = BC.e2e_inputs(E2E_SEED)
    dec, p = BC.decoder(c["M"], c["H"], c["V"], E2E_SEED, "cpu")
    oracle = [BC.oracle_caption(p, f, cap) for f, cap in items]
    args = types.SimpleNamespace(dataset=BC.ListDataset(items, c["V"]), print_freq=3, checkpoint=None)
    out = evaluate("cpu", args, BC.IdentityEncoder(), dec)
    assert len(out["losses"]) == 7
    for i, o in enumerate(oracle):
        assert o["gap"].min() >= 1e-4  # precondition: no near-tied argmax
        assert _close(out["losses"][i], o["loss"]), (i, out["losses"][i], o["loss"])
        assert out["references"][i] == [EC.strip(items[i][1], c["V"])] * o["n"]
        assert out["hypotheses"][i] == EC.strip(o["pred"], c["V"])


def test_e2e_case_has_the_margins_and_counts_it_claims():
    c = BC.E2E
    items = BC.e2e_inputs(E2E_SEED)
    p = BC.params(c["M"], c["H"], c["V"], E2E_SEED)
    oracle = [BC.oracle_caption(p, f, cap) for f, cap in items]
    assert sum(o["n"] for o in oracle) == 41
    assert min(o["gap"].min() for o in oracle) >= 1e-4 and min(o["margin"].min() for o in oracle) >= 1e-4
    assert sum(int((o["rank"] == 0).sum()) for o in oracle) == 2
    assert sum(int((o["rank"] < 5).sum()) for o in oracle) == 6


def test_rows_ref_offset_is_the_shared_contract():
    x, caps = EC.constructed(3, 3, 50, seed=4, L=6)
    for a, b in zip(BC.rows_ref(x, caps, [3, 1, 0], 1), EC.rows_ref(x, caps, [3, 1, 0])):
        assert np.array_equal(a, b)
    loss0, _, rank0 = BC.rows_ref(x, caps, None, 0)
    r = x[1, 2].astype(np.float64)
    tgt = caps[1, 2]
    assert rank0[1, 2] == int((r > r[tgt]).sum() + (r[:tgt] == r[tgt]).sum())
    assert abs(loss0[1, 2] - (np.log(np.exp(r - r.max()).sum()) + r.max() - r[tgt])) < 1e-12


def test_eval_cli_rebuilds_baseline_modules_from_a_state_dict(monkeypatch, tmp_path):
    import eval as E
    import models.baseline as MB
    from checkpoint import save_checkpoint
    from models.encoder import Encoder
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    M, H, V = 16, 24, 50
    dec, p = BC.decoder(M, H, V, 9, "cpu")
    opt = types.SimpleNamespace(state_dict=lambda: {})
    save_checkpoint(types.SimpleNamespace(model_name="tinyb"), 0, Encoder(M), dec, None, opt, {}, verbose=False)
    calls = []

    def fake(device, args, encoder, decoder):
        calls.append((device, args, encoder, decoder))
        return {"losses": [1.0]}

    monkeypatch.setattr(MB, "evaluate", fake)
    out = E.main(["tinyb_0.pth.tar", "--model_type", "baseline", "--batch_size", "4", "--synthetic_size", "6",
                  "--vocab_size", "50", "--synthetic_len", "8"])
    assert out == {"losses": [1.0]} and len(calls) == 1
    _, args, enc, got = calls[0]
    assert isinstance(got, MB.BaselineDecoder) and isinstance(enc, Encoder)
    assert (got.embed_size, got.hidden_size, got.linear.out_features) == (M, H, V)
    assert enc.embed.out_features == M and args.batch_size == 4
    for k, v in got.state_dict().items():
        assert torch.equal(v.cpu(), p[k]), k
    with pytest.raises(SystemError):  # the vocabulary must have the checkpoint's size
        E.main(["tinyb_0.pth.tar", "--model_type", "baseline", "--synthetic_size", "6", "--vocab_size", "51"])


def test_new_entry_points_are_declared_exported_and_bound():
    import os
    import re
    import capmi
    from capmi import kernels as K
    new = {"capmi_lstm_step_fwd", "capmi_eval_rows_at", "capmi_eval_captions_ce"}
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "capmi.h")
    with open(hdr) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in new:
        assert re.search(r"^int " + name + r"\(", text, flags=re.M), name
        assert hasattr(ctypes.CDLL(capmi.LIB_PATH), name)
    assert new <= set(capmi.EXPORTS)
    assert capmi.ABI_VERSION == capmi.lib.capmi_abi_version()
    assert callable(K.lstm_step_fwd) and callable(K.eval_rows_at) and callable(K.eval_captions_ce)


def test_new_entry_points_reject_bad_arguments():
    """CAPMI_EINVAL (1001) before any launch: runs without a GPU."""
    import capmi
    lib = capmi.lib
    buf = (ctypes.c_float * 256)()
    q = ctypes.cast(buf, ctypes.c_void_p).value
    q2, q3, q4 = q + 64, q + 128, q + 192
    # pre ld_pre x ld_x M h_prev ld_h c_prev ld_c w_ih w_hh b_ih b_hh R H h_out c_out stream
    ok = [None, 0, q, 16, 16, q2, 8, q2, 8, q, q, q, q, 2, 8, q3, q4, None]

    def bad(**kw):
        a = list(ok)
        for pos, v in kw.items():
            a[int(pos[1:])] = v
        return lib.capmi_lstm_step_fwd(*a)

    assert bad(p4=18, p3=20) == 1001            # M % 4 != 0
    assert bad(p14=6) == 1001                   # H % 4 != 0
    assert bad(p2=None, p5=None) == 1001        # none of pre / x / h_prev
    assert bad(p15=q2) == 1001                  # h_out == h_prev
    assert bad(p16=q2) == 1001                  # c_out == c_prev
    assert bad(p16=q3) == 1001                  # h_out == c_out
    assert bad(p13=0) == 1001 and bad(p14=0) == 1001
    assert bad(p2=q + 4) == 1001                # x not 16-byte aligned
    assert bad(p9=None) == 1001                 # x without W_ih
    assert bad(p15=None) == 1001
    # logits caps B T L V tgt_off lens loss_rows pred rank stream
    rows = [q, q, 2, 3, 3, 8, 0, None, q, q, None, None]
    for pos, v in ((0, None), (1, None), (8, None), (9, None), (2, 0), (3, 0), (5, 0), (6, -1), (6, 1), (4, 2)):
        a = list(rows)
        a[pos] = v
        assert lib.capmi_eval_rows_at(*a) == 1001, (pos, v)
    a = list(rows)
    a[4], a[6] = 4, 2                           # L = 4 < T + tgt_off = 5
    assert lib.capmi_eval_rows_at(*a) == 1001
    # loss_rows rank lens B T cap_ce cap_top1 cap_top5 stream
    cap = [q, q, None, 2, 3, q, q, q, None]
    for pos, v in ((0, None), (1, None), (5, None), (6, None), (7, None), (3, 0), (4, -1)):
        a = list(cap)
        a[pos] = v
        assert lib.capmi_eval_captions_ce(*a) == 1001, (pos, v)


def test_beam_helper_with_one_beam_is_greedy():
    M, H, V = 16, 24, 50
    start, end = V - 3, V - 2
    p = BC.decoder(M, H, V, 48, "cpu", fc_scale=60.0, end_bias=2.0, end_idx=end)[1]
    for i in range(3):
        feat = torch.from_numpy(gen.uniform(48 + i, "feats", (M,), -1, 1))
        b = BC.beam_loop(p, feat, 1, start, end, max_steps=20)
        seq, score, ended = BC.greedy_loop(p, feat, start, end, max_steps=20)
        if ended:
            assert b["ok"] and b["seq"] == seq and abs(b["done_scores"][0] - score) < 1e-4
        else:
            assert not b["ok"] and b["live_seqs"] == [seq]


def test_baseline_beam_search_limits():
    from capmi.beam import BaselineBatchedBeamSearch
    dec = types.SimpleNamespace()
    for k in (0, 17):
        with pytest.raises(ValueError):
            BaselineBatchedBeamSearch(dec, k)
    with pytest.raises(RuntimeError):
        BaselineBatchedBeamSearch(dec, 3).search(torch.zeros(1, 16), 1, 2)
