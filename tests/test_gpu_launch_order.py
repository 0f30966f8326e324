"""GPU: the libcapmi entry points every caller of a decoder's recurrence issues, in order.

``capmi.kernels.call`` is wrapped by a recorder that notes the entry point's name and calls through; each
caller runs once at the smallest shape that takes every branch of its sequence, and the names are compared with
lists written out here. B = 2 images, 3 beams or samples each, max_steps = 2 (three decode steps, ``sync_every``
above that, so the loop length is fixed); captions of L = 4 tokens for the teacher-forced callers."""
import pytest
import torch

import baseline_cases as BLC
import beam_cases as BC
import gen
from helpers import t

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, START, END = 120, 117, 118
BL_M, BL_H, BL_V = 16, 24, 50
STEPS, L = 3, 4

GEMM, SK = "capmi_gemm", "capmi_gemm_sk_ex"
ATT_SETUP = [GEMM, "capmi_mean_rows", GEMM]
ATT_STEP = ["capmi_embed_gather", GEMM, "capmi_beam_att_fwd", GEMM, "capmi_lstm_cell_fwd", GEMM]
BL_SETUP = ["capmi_lstm_step_fwd"]
BL_STEP = ["capmi_embed_gather", "capmi_lstm_step_fwd", GEMM]
BEAM = ["capmi_beam_select", "capmi_beam_advance"]
SAMPLE = ["capmi_sample_step"]
# the teacher-forced forward: X[1:] gather, hoisted input GEMM, T steps, vocabulary GEMM
FWD_UNFUSED = (["capmi_embed_gather", SK, "capmi_lstm_cell_fwd"] + [GEMM, "capmi_lstm_cell_fwd"] * (L - 1) + [SK])
# dH, dW_lin, db_lin, BPTT, dW_ih, dW_hh, the bias column sum, dX, the embedding scatter-add
BWD_HEAD, BWD_TAIL = [SK, SK, "capmi_colsum"], [SK, SK, "capmi_colsum", SK, "capmi_embed_scatter_add"]
BWD_UNFUSED = BWD_HEAD + ["capmi_lstm_cell_bwd"] + [GEMM, "capmi_lstm_cell_bwd"] * (L - 1) + BWD_TAIL
LOSS = ["capmi_count_targets", "capmi_ce_ignore_fwd_bwd", "capmi_loss_finalize_dev"]


@pytest.fixture
def calls(monkeypatch):
    from capmi import kernels as K
    names, through = [], K.call

    def recorder(name, *args):
        names.append(name)
        return through(name, *args)

    monkeypatch.setattr(K, "call", recorder)
    return names


@pytest.fixture(scope="module")
def attention():
    dec, _ = BC.tuned_decoder(64, 48, 32, V, 62, 1.0, 0.0, END, DEV)
    return dec, BC.features((62, 162)).to(DEV)


@pytest.fixture(scope="module")
def baseline():
    dec, _ = BLC.decoder(BL_M, BL_H, BL_V, 48, DEV)
    feats = torch.stack([t(gen.uniform(48 + i, "feats", (BL_M,), -1, 1)) for i in range(2)]).to(DEV)
    caps = torch.randint(1, BL_V, (2, L), generator=torch.Generator().manual_seed(7)).to(DEV)
    return dec, feats, caps


@pytest.mark.parametrize("return_alphas", [True, False])
def test_batched_beam_search(calls, attention, return_alphas):
    from capmi.beam import BatchedBeamSearch
    dec, feats = attention
    bs = BatchedBeamSearch(dec, 3)
    bs.search(feats, START, END, max_steps=STEPS - 1, return_alphas=return_alphas, sync_every=100)
    assert bs.last_stats["steps"] == STEPS
    assert calls == ATT_SETUP + (ATT_STEP + BEAM) * STEPS


def test_batched_sampler(calls, attention):
    from capmi.sample import BatchedSampler
    dec, feats = attention
    s = BatchedSampler(dec, 3)
    s.sample(feats, START, END, max_steps=STEPS - 1, seed=1, sync_every=100)
    assert s.last_stats["steps"] == STEPS
    assert calls == ATT_SETUP + (ATT_STEP + SAMPLE) * STEPS


def test_baseline_batched_beam_search(calls, baseline):
    from capmi.beam import BaselineBatchedBeamSearch
    dec, feats, _ = baseline
    bs = BaselineBatchedBeamSearch(dec, 3)
    bs.search(feats, BL_V - 3, BL_V - 2, max_steps=STEPS - 1, sync_every=100)
    assert bs.last_stats["steps"] == STEPS
    assert calls == BL_SETUP + (BL_STEP + BEAM) * STEPS


def test_baseline_batched_sampler(calls, baseline):
    from capmi.sample import BaselineBatchedSampler
    dec, feats, _ = baseline
    s = BaselineBatchedSampler(dec, 3)
    s.sample(feats, BL_V - 3, BL_V - 2, max_steps=STEPS - 1, seed=1, sync_every=100)
    assert s.last_stats["steps"] == STEPS
    assert calls == BL_SETUP + (BL_STEP + SAMPLE) * STEPS


@pytest.mark.parametrize("fused", [True, False])
def test_baseline_teacher_forced_eval(calls, baseline, monkeypatch, fused):
    from capmi import baseline_eval
    dec, feats, caps = baseline
    monkeypatch.setattr(baseline_eval, "STEP_FUSED", fused)
    baseline_eval.BaselineTeacherForcedEval(dec)(feats, caps, [L, L - 1])
    forward = ["capmi_embed_gather", SK] + ["capmi_lstm_step_fwd"] * L + [SK] if fused else FWD_UNFUSED
    assert calls == forward + ["capmi_eval_rows_at", "capmi_eval_captions_ce"]


def test_baseline_forward_and_backward(calls, baseline):
    from capmi.baseline_fn import baseline_forward
    dec, feats, caps = baseline
    dec.zero_grad()
    baseline_forward(dec, feats, caps).sum().backward()
    assert all(q.grad is not None for q in dec.parameters())
    dec.zero_grad()
    assert calls == FWD_UNFUSED + BWD_UNFUSED


@pytest.mark.parametrize("fused", [True, False])
def test_baseline_train_step_eager(calls, baseline, fused):
    from capmi.baseline_train import BaselineTrainStep
    from capmi.optim import Adam
    _, feats, caps = baseline
    dec, _ = BLC.decoder(BL_M, BL_H, BL_V, 48, DEV)  # its own: the optimizer takes the gradients over
    step = BaselineTrainStep(torch.nn.Identity(), dec, Adam(list(dec.parameters()), lr=1e-4))
    step.fused_fwd = step.fused_bwd = fused
    del calls[:]
    step(feats, caps, update=False)
    assert step.counts["eager"] == 1
    if fused:
        forward = ["capmi_embed_gather", SK] + ["capmi_lstm_step_fwd_train"] * L + [SK]
        backward = BWD_HEAD + ["capmi_lstm_step_bwd"] * L + BWD_TAIL
    else:
        forward, backward = FWD_UNFUSED, BWD_UNFUSED
    assert calls == forward + LOSS + backward
