"""CPU: the sampler's reference (tests/sample_cases.py::pick_ref) on hand-worked cases, the argument checks of
capmi.sample and capmi_sample_step (made before any launch, so without a GPU), and the new export."""
import math
import os
import re

import pytest
import torch

import sample_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# probabilities 1/8, 2/8, 4/8, 1/8: cdf 0.125, 0.375, 0.875, 1
L4 = torch.log(torch.tensor([1.0, 2.0, 4.0, 1.0]))


def test_pick_ref_hand_worked():
    tok, logp, margin = SC.pick_ref(L4, 0.5, 1.0, 0)
    assert tok == 2 and logp == pytest.approx(math.log(0.5), abs=1e-7) and margin == pytest.approx(0.125, abs=1e-7)
    tok, logp, margin = SC.pick_ref(L4, 0.9, 1.0, 0)
    assert tok == 3 and logp == pytest.approx(math.log(0.125), abs=1e-7) and margin == pytest.approx(0.025, abs=1e-7)
    # u = 0: the first entry with weight; u on a cdf value: strictly above it, so the next entry
    tok, logp, margin = SC.pick_ref(L4, 0.0, 1.0, 0)
    assert tok == 0 and logp == pytest.approx(math.log(0.125), abs=1e-7) and margin == 0.0
    assert SC.pick_ref(torch.tensor([0.0, 0.0]), 0.5, 1.0, 0)[0] == 1
    # top_k = 2 keeps {2, 1}: probabilities 0, 1/3, 2/3, 0
    tok, logp, margin = SC.pick_ref(L4, 0.2, 1.0, 2)
    assert tok == 1 and logp == pytest.approx(math.log(1 / 3), abs=1e-7)
    assert margin == pytest.approx(1 / 3 - 0.2, abs=1e-7)
    assert SC.pick_ref(L4, 0.0, 1.0, 2)[0] == 1  # entry 0 is not kept: never drawn
    assert SC.pick_ref(L4, 0.99, 1.0, 2)[0] == 2  # nor entry 3
    assert SC.pick_ref(L4, 0.99, 1.0, 4)[0] == 3 and SC.pick_ref(L4, 0.99, 1.0, 9)[0] == 3  # top_k >= V: all
    # temperature 0.5 squares the ratios: 1/16, 1/4, 1, 1/16 over 1.375
    tok, logp, _ = SC.pick_ref(L4, 0.1, 0.5, 0)
    assert tok == 1 and logp == pytest.approx(math.log(0.25 / 1.375), abs=1e-7)
    # greedy: argmax, the lower index on a tie, log_softmax at temperature 1, u and top_k ignored
    tok, logp, margin = SC.pick_ref(L4, 0.99, 0.0, 1)
    assert tok == 2 and logp == pytest.approx(math.log(0.5), abs=1e-7) and margin == float("inf")
    assert SC.pick_ref(torch.tensor([1.0, 3.0, 3.0, 0.0]), 0.5, 0.0, 0)[0] == 1
    # a tie across the top-k threshold keeps the lower index; -inf carries no weight
    assert SC.kept_mask(torch.tensor([1.0, 3.0, 3.0, 0.0]), 1).tolist() == [False, True, False, False]
    inf = float("inf")
    assert SC.pick_ref(torch.tensor([-inf, 2.0, -inf, 1.0]), 0.0, 1.0, 0)[0] == 1
    assert SC.pick_ref(torch.tensor([-inf, 2.0, -inf, 1.0]), 1 - 2.0 ** -24, 1.0, 3)[0] == 3
    assert SC.logp_fp32(L4, 2, 1.0, 0) == pytest.approx(math.log(0.5), abs=1e-6)


@pytest.mark.parametrize("cls", ["BatchedSampler", "BaselineBatchedSampler"])
def test_constructor_rejects_bad_arguments(cls):
    import capmi.sample as S
    ctor = getattr(S, cls)
    for args in ((0,), (-1,), (1, -0.5), (1, float("nan")), (1, 1.0, -1)):
        with pytest.raises(ValueError):
            ctor(None, *args)
    s = ctor(None, 3, 0.0, 7)
    assert (s.n, s.temperature, s.top_k) == (3, 0.0, 7)
    assert ctor(None).n == 1 and ctor(None).temperature == 1.0 and ctor(None).top_k == 0


def test_attention_sampler_is_bounded_by_the_attention_kernel_rows():
    from capmi.sample import BatchedSampler
    BatchedSampler(None, 16)
    with pytest.raises(ValueError):
        BatchedSampler(None, 17)


def test_sample_step_rejects_bad_calls_before_any_launch():
    from capmi._lib import lib
    ok = 256  # a non-null stand-in: validation never dereferences it
    assert lib.capmi_sample_step(None, 8, 1, 8, None, 1.0, 0, 7, 0, None, None, None, None, None, None) == 1001
    for missing in range(7):
        ptrs = [ok] * 7
        ptrs[missing] = None
        logits, u, alive, prev, tokens, logp, rows_live = ptrs
        assert lib.capmi_sample_step(logits, 8, 1, 8, u, 1.0, 0, 7, 0, alive, prev, tokens, logp, rows_live,
                                     None) == 1001

    def call(ld=8, R=1, V=8, temperature=1.0, top_k=0, step=0):
        return lib.capmi_sample_step(ok, ld, R, V, ok, temperature, top_k, 7, step, ok, ok, ok, ok, ok, None)

    assert call(R=0) == 1001 and call(V=0) == 1001 and call(ld=7) == 1001
    assert call(temperature=-1.0) == 1001 and call(temperature=float("nan")) == 1001
    assert call(top_k=-1) == 1001 and call(step=-1) == 1001


def test_export_is_declared_and_bound():
    import capmi
    src = open(os.path.join(REPO, "include", "capmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"^int\s+capmi_sample_step\s*\(", src, flags=re.M)
    assert "capmi_sample_step" in capmi.EXPORTS
    assert hasattr(capmi.lib, "capmi_sample_step")
    from capmi import kernels as K
    with pytest.raises(ValueError):  # device tensors only, like every wrapper
        z = torch.zeros(1, 4)
        i = torch.zeros(1, dtype=torch.int32)
        K.sample_step(z, 1, 4, torch.zeros(1), 1.0, 0, 3, 0, i, torch.zeros(1, dtype=torch.int64), i, torch.zeros(1), i)


def test_gen_captions_surface_defaults():
    import types

    import gen_captions as G
    assert G._sample_args(types.SimpleNamespace()) == (1, 1.0, 0, None)
    assert G._sample_args(types.SimpleNamespace(num_samples=5, temperature=0.7, top_k=10, seed=3)) == (5, 0.7, 10, 3)
    assert callable(G.caption_images_sample) and callable(G.baseline_caption_images_sample)
