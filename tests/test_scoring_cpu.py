"""CPU: capmi.scoring.caption_scores against the scores of the reference project's BLEU / ROUGE-L / CIDEr
scorers (tests/golden/caption_scores.json, written by tests/golden/make_scores_golden.py) and against
hand-computed cases."""
import json
import math
import os

import pytest

from capmi.scoring import bleu, caption_scores, cider, rouge_l

KEYS = ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "caption_scores.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", ["corpus", "single_image"])
def test_matches_the_reference_scorers(fixture, case):
    """Both sides evaluate the same formulas in fp64 and differ by summation order only: 1e-9 relative."""
    c = fixture[case]
    got = caption_scores(c["references"], c["hypotheses"])
    assert sorted(got) == sorted(KEYS) and "METEOR" not in got
    for k in KEYS:
        want = c["scores"][k]
        assert isinstance(got[k], float) and abs(got[k] - want) <= 1e-9 * abs(want), (k, got[k], want)


def test_fixture_covers_the_edge_cases(fixture):
    c = fixture["corpus"]
    refs, hyps = c["references"], c["hypotheses"]
    assert len(hyps) >= 36 and len(refs) == len(hyps)
    assert any(len(h) == 0 for h in hyps) and any(0 < len(h) < 4 for h in hyps)
    assert any(h == r[0] for h, r in zip(hyps, refs))  # an exact match
    # the reference's quirk: one copy of the stripped target per target position (its words + END)
    assert sum(1 for r in refs if all(x == r[0] for x in r) and len(r) == len(r[0]) + 1) >= 30
    assert any(len({tuple(x) for x in r}) > 1 for r in refs)  # and genuinely different references
    assert len(fixture["single_image"]["hypotheses"]) == 1


def test_perfect_match_scores_one():
    refs = [[[4, 5, 6, 7, 8]] * 6, [[9, 10, 11, 12]] * 5]
    hyps = [[4, 5, 6, 7, 8], [9, 10, 11, 12]]
    s = caption_scores(refs, hyps)
    for k in KEYS[:5]:
        assert abs(s[k] - 1.0) < 1e-8, (k, s[k])
    assert s["CIDEr"] > 0


def test_disjoint_vocabularies_score_zero():
    refs = [[[1, 2, 3, 4]], [[5, 6, 7]]]
    hyps = [[11, 12, 13, 14], [15, 16, 17]]
    s = caption_scores(refs, hyps)
    assert s["ROUGE_L"] == 0.0 and s["CIDEr"] == 0.0 and s["Bleu_1"] < 1e-12


def test_bleu_by_hand():
    """hyp 1 2 3 4 9 against 1 2 3 4 5 6: unigrams 4/5, bigrams 3/4, trigrams 2/3, 4-grams 1/2, brevity exp(1 - 6/5)."""
    b = bleu([[[1, 2, 3, 4, 5, 6]]], [[1, 2, 3, 4, 9]])
    bp = math.exp(1 - 6 / 5)
    want = [0.8, (0.8 * 0.75) ** 0.5, (0.8 * 0.75 * 2 / 3) ** (1 / 3), (0.8 * 0.75 * 2 / 3 * 0.5) ** 0.25]
    for got, w in zip(b, want):
        assert abs(got - w * bp) < 1e-8
    # counts are clipped by the reference's: 7 7 7 against one 7 is 1/3
    assert abs(bleu([[[7, 8, 9]]], [[7, 7, 7]])[0] - 1 / 3) < 1e-8
    # the closest reference length sets the brevity penalty, the shorter one on a tie: no penalty at 3 vs (3, 7)
    assert abs(bleu([[[1, 2, 3], [1, 2, 3, 4, 5, 6, 7]]], [[1, 2, 3, 4, 5]])[0] - 1.0) < 1e-8


def test_rouge_l_by_hand():
    """LCS(1 2 3 4, 1 9 3 4 5) = 3: precision 3/5, recall 3/4, F with beta = 1.2."""
    p, r, b2 = 3 / 5, 3 / 4, 1.2 ** 2
    assert abs(rouge_l([[[1, 2, 3, 4]]], [[1, 9, 3, 4, 5]]) - (1 + b2) * p * r / (r + b2 * p)) < 1e-12
    assert rouge_l([[[1, 2, 3]]], [[]]) == 0.0  # an empty hypothesis matches nothing
    # best precision and best recall may come from different references
    got = rouge_l([[[1, 2], [1, 2, 3, 4, 5, 6]]], [[1, 2, 3]])
    assert abs(got - (1 + b2) * 1.0 * 1.0 / (1.0 + b2 * 1.0)) < 1e-12


def test_cider_by_hand():
    """Two images; an n-gram in both reference sets has IDF log(2) - log(2) = 0, one in a single set log(2)."""
    refs = [[[1, 2]], [[1, 3]]]
    s = cider(refs, [[1, 2], [1, 3]])
    # per image: unigram and bigram vectors match exactly (cosine 1), no 3-/4-grams: mean over n = 2/4, x10
    assert abs(s - 5.0) < 1e-12
    assert cider(refs, [[1], [1]]) == 0.0  # the shared word alone carries no weight


def test_rejects_mismatched_inputs():
    with pytest.raises(ValueError):
        caption_scores([[[1]]], [[1], [2]])
    with pytest.raises(ValueError):
        caption_scores([[]], [[1]])
