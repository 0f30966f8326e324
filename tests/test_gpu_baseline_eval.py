"""GPU: models.baseline.evaluate_batched and capmi.baseline_eval.BaselineTeacherForcedEval against the fp64
oracle of every caption alone (tests/baseline_cases.py) and against the batch-1 ``evaluate`` loop, and eval.py
end to end on a baseline checkpoint.

The case (seed 75, M = 16, H = 24, V = 50, 7 captions of lengths [5, 8, 3, 6, 4, 8, 7] = 41 rows) was chosen
on the CPU with the fp64 oracle alone: least top-2 logit gap 4.9e-4, least distance of a target's logit from
any other 2.4e-4, both far above fp32 rounding of O(0.3) logits over K = 24, so no row is left out: every token
and every count is compared exactly. 2 top-1 and 6 top-5 hits."""
import json
import math
import types

import pytest
import torch

import baseline_cases as BC
import eval_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
E2E_SEED = 75


def _close(got, want):
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


@pytest.fixture(scope="module")
def e2e():
    """The 7 captions, the decoder, the per-caption fp64 oracle and the batch-1 evaluate run on the GPU."""
    from models.baseline import evaluate
    c = BC.E2E
    dec, p = BC.decoder(c["M"], c["H"], c["V"], E2E_SEED, DEV)
    items = BC.e2e_inputs(E2E_SEED)
    oracle = [BC.oracle_caption(p, f, cap) for f, cap in items]
    assert min(o["gap"].min() for o in oracle) >= 1e-4 and min(o["margin"].min() for o in oracle) >= 1e-4
    dataset = BC.ListDataset(items, c["V"])
    args = types.SimpleNamespace(dataset=dataset, print_freq=3, checkpoint=None)
    single = evaluate(DEV, args, BC.IdentityEncoder(), dec)
    return dict(dec=dec, items=items, oracle=oracle, args=args, dataset=dataset, single=single)


def test_evaluate_batched_matches_oracle_and_batch_1_loop(e2e):
    from models.baseline import evaluate_batched
    c, V = BC.E2E, BC.E2E["V"]
    items, oracle, single = e2e["items"], e2e["oracle"], e2e["single"]
    lengths = [len(cap) for _, cap in items]
    assert lengths == c["lengths"] and lengths != sorted(lengths, reverse=True) and len(items) % c["batch_size"] != 0
    out = evaluate_batched(DEV, e2e["args"], BC.IdentityEncoder(), e2e["dec"], dataset=e2e["dataset"],
                           batch_size=c["batch_size"])
    assert evaluate_batched.last_eval.last_stats["host_syncs"] == 0
    assert len(out["losses"]) == len(single["losses"]) == 7
    for i, o in enumerate(oracle):
        print(f"caption {i}: batched {out['losses'][i]:.8f} batch-1 {single['losses'][i]:.8f} oracle {o['loss']:.8f} "
              f"min gap {o['gap'].min():.3g} min target margin {o['margin'].min():.3g}")
        assert _close(out["losses"][i], o["loss"])
        assert _close(out["losses"][i], single["losses"][i])
        assert out["references"][i] == single["references"][i] == [EC.strip(items[i][1], V)] * o["n"]
        assert out["hypotheses"][i] == single["hypotheses"][i] == EC.strip(o["pred"], V)
    rows = sum(lengths)
    assert rows == 41 and round(out["top1_acc"] * rows, 9) == 2 and round(out["top5_acc"] * rows, 9) == 6
    assert sum(int((o["rank"] == 0).sum()) for o in oracle) == 2
    assert sum(int((o["rank"] < 5).sum()) for o in oracle) == 6
    assert _close(out["loss"], sum(l * n for l, n in zip(out["losses"], lengths)) / rows)
    for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"):
        assert math.isfinite(out[k])
    assert "METEOR" not in out
    assert json.loads(json.dumps(out)) == out


def test_evaluate_dispatches_on_the_batch_size(e2e):
    from models.baseline import evaluate
    args = types.SimpleNamespace(dataset=e2e["dataset"], print_freq=3, checkpoint=None, batch_size=4)
    out = evaluate(DEV, args, BC.IdentityEncoder(), e2e["dec"])
    assert "top1_acc" in out and len(out["losses"]) == 7


def test_teacher_forced_eval_returns_the_callers_order(e2e):
    """One call over all 7 captions in dataset (unsorted) order, and again in another order: the same
    per-caption numbers, each at the position the caller gave it; nothing is read back inside the call."""
    from torch.nn.utils.rnn import pad_sequence
    from capmi.baseline_eval import BaselineTeacherForcedEval, unpack
    items, oracle = e2e["items"], e2e["oracle"]
    tf = BaselineTeacherForcedEval(e2e["dec"])

    def run(order):
        feats = torch.stack([items[i][0] for i in order]).to(DEV)
        caps = pad_sequence([items[i][1] for i in order], batch_first=True, padding_value=0).to(DEV)
        res = tf(feats, caps, [len(items[i][1]) for i in order])
        stats = dict(tf.last_stats)
        torch.cuda.synchronize()
        return res, stats

    order = list(range(7))
    res, stats = run(order)
    T = 8
    assert stats == {"launches": 2, "host_syncs": 0, "step_launches": T}
    other = [3, 6, 0, 5, 2, 1, 4]
    res2, _ = run(other)
    assert res["lengths"] == [o["n"] for o in oracle]
    assert res["pred"].shape == (7, T) and res["pred"].dtype == I32 and res["top1"].dtype == I32
    again = unpack(res["packed"].cpu(), 7, T)
    for i, o in enumerate(oracle):
        n, j = o["n"], other.index(i)
        assert _close(float(res["cap_loss"][i]), o["loss"])
        assert _close(float(res2["cap_loss"][j]), o["loss"])
        assert res["pred"][i, :n].tolist() == o["pred"].tolist() and (res["pred"][i, n:] == -1).all()
        assert res2["pred"][j].tolist() == res["pred"][i].tolist()
        assert int(res["top1"][i]) == int((o["rank"] == 0).sum()) and int(res["top5"][i]) == int((o["rank"] < 5).sum())
        assert int(res2["top1"][j]) == int(res["top1"][i]) and int(res2["top5"][j]) == int(res["top5"][i])
        assert float(again["cap_loss"][i]) == float(res["cap_loss"][i])
    with pytest.raises(ValueError):
        tf(torch.zeros(1, 16, device=DEV), torch.zeros(1, 4, dtype=torch.int64, device=DEV), [1])
    with pytest.raises(ValueError):
        tf(torch.zeros(1, 16, device=DEV), torch.zeros(1, 4, dtype=torch.int64, device=DEV), [5])


def test_fused_and_three_launch_step_give_the_same_captions(e2e, monkeypatch):
    """The step sequence stays selectable (capmi.baseline_eval.STEP_FUSED): both give the oracle's tokens."""
    from torch.nn.utils.rnn import pad_sequence
    from capmi import baseline_eval
    items, oracle = e2e["items"], e2e["oracle"]
    feats = torch.stack([f for f, _ in items]).to(DEV)
    caps = pad_sequence([cap for _, cap in items], batch_first=True, padding_value=0).to(DEV)
    monkeypatch.setattr(baseline_eval, "STEP_FUSED", False)
    tf = baseline_eval.BaselineTeacherForcedEval(e2e["dec"])
    res = tf(feats, caps, [len(cap) for _, cap in items])
    torch.cuda.synchronize()
    assert tf.last_stats["step_launches"] == 2 * 8 - 1
    for i, o in enumerate(oracle):
        assert _close(float(res["cap_loss"][i]), o["loss"])
        assert res["pred"][i, :o["n"]].tolist() == o["pred"].tolist()


def test_eval_cli_end_to_end(tmp_path, monkeypatch):
    """eval.main through the real Encoder on 6 synthetic ragged captions, batch 4, from a checkpoint written by
    save_checkpoint: 6 finite losses, and the JSON it writes equals the return."""
    import eval as E
    from checkpoint import save_checkpoint
    from models.encoder import Encoder
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    dec, _ = BC.decoder(16, 24, 50, 9, "cpu")
    opt = types.SimpleNamespace(state_dict=lambda: {})
    save_checkpoint(types.SimpleNamespace(model_name="tinyb"), 0, Encoder(16), dec, None, opt, {}, verbose=False)
    out = E.main(["tinyb_0.pth.tar", "--model_type", "baseline", "--batch_size", "4", "--synthetic_size", "6",
                  "--vocab_size", "50", "--synthetic_len", "8", "--print_freq", "10"])
    assert len(out["losses"]) == 6 and all(math.isfinite(x) for x in out["losses"])
    assert 0.0 <= out["top1_acc"] <= out["top5_acc"] <= 1.0
    with open(tmp_path / "eval_data" / "tinyb_0.json") as f:
        assert json.load(f) == out
