"""CPU: the host side of validation on generated captions (capmi.genval): the corpus formulas on accumulated rows,
the per-image dataset view, eval.py's new flags and the argument checks that need no device."""
import math
import types

import numpy as np
import pytest
import torch

import score_cases as S

# three images scored by hand: references, the hypothesis, and its CAPMI_SCORE_STATS integers (matches 1..4,
# guesses 1..4, hypothesis length, closest reference length, lcs_p, lcs_r, len_r, ROUGE-L's hypothesis length)
HAND = [
    ([[5, 6, 7, 8], [5, 9, 7]], [5, 6, 7], [3, 2, 1, 0, 3, 2, 1, 0, 3, 3, 3, 3, 4, 3]),
    ([[4, 5, 6], [4, 5, 6, 7, 8]], [4, 5, 5, 6], [3, 2, 0, 0, 4, 3, 2, 1, 4, 3, 3, 3, 3, 4]),
    ([[9, 9, 8], [7]], [9, 8], [2, 1, 0, 0, 2, 1, 0, 0, 2, 1, 2, 2, 3, 2]),
]


def test_corpus_scores_from_rows_on_hand_made_rows():
    from capmi.devscore import corpus_scores_from_rows
    from capmi.scoring import caption_scores
    refs, hyps, rows = (list(x) for x in zip(*HAND))
    for r, h, row in HAND:  # the hand-made rows are capmi.scoring's counting
        assert S.row_integers(r, h) == row
    cider = np.array([0.25, 1.5, 3.0625], dtype=np.float32)
    want = caption_scores(refs, hyps)
    for stats in (np.array(rows, dtype=np.int32), np.array(rows, dtype=np.int64), rows):
        got = corpus_scores_from_rows(stats, cider)
        assert set(got) == set(want) and all(isinstance(v, float) for v in got.values())
        for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L"):
            assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
        assert got["CIDEr"] == math.fsum([0.25, 1.5, 3.0625]) / 3
    # one image's rows in any order of accumulation: the sums are integers, the ROUGE-L mean an exact fsum
    back = corpus_scores_from_rows(np.array(rows[::-1]), cider[::-1])
    assert back == got
    for bad in (np.zeros((3, 13), np.int32), np.zeros((0, 14), np.int32)):
        with pytest.raises(ValueError):
            corpus_scores_from_rows(bad, np.zeros(bad.shape[0], np.float32))
    with pytest.raises(ValueError):
        corpus_scores_from_rows(np.array(rows), cider[:2])


def test_corpus_scores_goes_through_corpus_scores_from_rows(monkeypatch):
    """``DeviceCaptionScorer.corpus_scores`` ends in the new function: with the device part stubbed it hands over the
    rows it got and returns what comes back."""
    from capmi import devscore
    seen = {}

    def fake_rows(stats, cider):
        seen["stats"], seen["cider"] = np.asarray(stats), np.asarray(cider)
        return {"sentinel": 1.0}

    rows = np.array([h[2] for h in HAND], dtype=np.int32)
    scorer = devscore.DeviceCaptionScorer.__new__(devscore.DeviceCaptionScorer)
    scorer.refs = types.SimpleNamespace(n_images=3, device=torch.device("cpu"))
    scorer.score_table = lambda tokens, lens, img_key: {"stats": torch.from_numpy(rows),
                                                        "cider": torch.tensor([1.0, 2.0, 3.0])}
    monkeypatch.setattr(devscore, "corpus_scores_from_rows", fake_rows)
    assert scorer.corpus_scores([h[1] for h in HAND]) == {"sentinel": 1.0}
    assert np.array_equal(seen["stats"], rows) and seen["cider"].tolist() == [1.0, 2.0, 3.0]


def test_eval_flags():
    import eval as E
    a = E.parse_args(["c.pth.tar", "--model_type", "attention"])
    assert (a.decode, a.beam_size, a.max_decode_len, a.length_alpha) == ("teacher", 3, 50, 0.0)
    a = E.parse_args(["c.pth.tar", "--model_type", "baseline", "--decode", "beam", "--beam_size", "5",
                      "--max_decode_len", "20", "--length_alpha", "0.7", "--synthetic_size", "13", "--batch_size", "4"])
    assert (a.decode, a.beam_size, a.max_decode_len, a.length_alpha) == ("beam", 5, 20, 0.7)
    assert a.synthetic_size == 13 and a.batch_size == 4
    with pytest.raises(SystemExit):
        E.parse_args(["c.pth.tar", "--model_type", "attention", "--decode", "greedy"])


@pytest.mark.parametrize("model", ["attention", "baseline"])
def test_evaluate_generated_needs_a_hip_device(model):
    import importlib
    mod = importlib.import_module(f"models.{model}")
    args = types.SimpleNamespace(beam_size=3, max_decode_len=50, length_alpha=0.0, print_freq=1)
    with pytest.raises(RuntimeError):
        mod.evaluate_generated(torch.device("cpu"), args, None, None)


def test_max_decode_len_is_bounded_by_the_scorer():
    from capmi.devscore import ScoreRefs
    from capmi.genval import GeneratedCaptionEval
    refs = ScoreRefs.build([[[3, 4, 5]]])
    with pytest.raises(ValueError):
        GeneratedCaptionEval(None, None, None, refs, 47, 48, 0, max_decode_len=64)
    with pytest.raises(ValueError):
        GeneratedCaptionEval(None, None, None, refs, 47, 48, 0, max_decode_len=-1)
    with pytest.raises(ValueError):  # tables that append END would count it against captions that carry none
        GeneratedCaptionEval(None, None, None, ScoreRefs.build([[[3, 4, 5]]], end_idx=48), 47, 48, 0)
    ev = GeneratedCaptionEval(None, None, None, refs, 47, 48, 0, max_decode_len=63)  # the tables, on the host here
    assert ev.tokens.shape == (64, 1) and ev.stats.shape == (1, 14) and int(ev.tokens.max()) == -1
    for keys in ([1], [0, 2], [-1]):  # a batch fills one slice of the tables: consecutive keys inside them
        with pytest.raises(ValueError):
            ev.step(None, keys)


def test_per_image_view_of_synthetic_coco():
    from capmi.data import SyntheticCOCO
    from capmi.genval import PerImageView, build_refs
    ds = SyntheticCOCO(13, V=50, L=8, ragged=True)
    view = PerImageView(ds)
    assert len(view) == 13 and view.keys == list(range(13)) and view.vocab is ds.vocab
    for i in (0, 5, 12):
        img, key = view[i]
        assert key == i and torch.equal(img, ds[i][0])
        got, want = view.references(key), ds.references(i)
        assert len(got) == len(want) == 5 and all(torch.equal(a, b) for a, b in zip(got, want))
    start, end, pad = 47, 48, 0
    refs, listed = build_refs(view, {start, end, pad}, "cpu")
    assert refs.n_images == 13 and refs.end_idx is None
    assert listed[3][0] == ds[3][1][1:-1].tolist()  # the item's own caption first, START / END stripped
    assert all(w not in (start, end, pad) for caps in listed for c in caps for w in c)


def test_per_image_view_of_a_dataset_with_img_ids():
    """COCODataset's surface: one item per image in ``img_ids`` order although the dataset lists one item per caption."""
    from capmi.genval import PerImageView

    class Stub:
        vocab = "v"
        img_ids = [11, 22, 33]

        def __len__(self):
            return 7  # captions

        def _get_transformed_img(self, img_id):
            return f"img{img_id}"

        def references(self, key):
            return [torch.tensor([key])]

    view = PerImageView(Stub())
    assert len(view) == 3 and [view[i] for i in range(3)] == [("img11", 0), ("img22", 1), ("img33", 2)]
    assert view.references(2)[0].tolist() == [2]


def test_backtrack_rejects_bad_arguments_before_any_launch():
    """capmi_beam_backtrack's checks need no device: every pointer below is a stand-in that is never read."""
    from capmi._lib import lib
    EINVAL, ERANGE = 1001, 1003
    p = 256

    def call(bp=p, tokens=p, steps=3, B=5, k=3, T=7, end=48, alpha=0.0, rows=None):
        return lib.capmi_beam_backtrack(bp, p, p, p, p, p, p, steps, B, k, T, end, -1, -1, 0, 0, alpha, tokens, p, p, p,
                                        rows, None)

    assert call(bp=None) == EINVAL and call(tokens=None) == EINVAL
    assert call(B=0) == EINVAL and call(k=0) == EINVAL and call(k=17) == EINVAL and call(T=0) == EINVAL
    assert call(steps=-1) == EINVAL and call(steps=8) == EINVAL and call(end=-1) == EINVAL
    assert call(alpha=-0.5) == EINVAL and call(alpha=float("nan")) == EINVAL
    assert call(B=1 << 24, k=16, T=3, steps=3) == ERANGE  # T * R * 3 = 9 * 2^28 >= 2^31
    assert call(B=(1 << 31) - 1, k=16, T=(1 << 31) - 1, steps=0) == ERANGE
