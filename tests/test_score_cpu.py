"""CPU: the host side of the device caption metrics (capmi.devscore, csrc/score.hip): the reference tables against a
brute-force build, their limits, the exports, the C entries' argument checks before any launch, the oracle of
tests/score_cases.py against the reference scorers' fixture, and the new keywords' plumbing."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import score_cases as S

EINVAL, ERANGE = 1001, 1003
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capmi_caption_stats", "capmi_reward_mix")


@pytest.fixture(scope="module")
def cases():
    return S.build_cases()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(REPO, "tests", "golden", "caption_scores.json")) as f:
        return json.load(f)


def test_the_cases_cover_every_shape_and_edge(cases):
    S.check_coverage(cases)
    again = S.build_cases()  # seeded
    assert [c["hyps"] for c in again] == [c["hyps"] for c in cases]


@pytest.mark.parametrize("end_idx", [None, S.END])
def test_tables_equal_a_brute_force_build(cases, end_idx):
    from capmi.devscore import ScoreRefs
    from capmi.scst import CiderRefs
    corpus = cases[0]["references"]
    refs = ScoreRefs.build(corpus, end_idx=end_idx)
    h = refs.host
    assert {k: v.dtype for k, v in h.items()} == dict(
        bleu_keys=np.uint64, bleu_cnt=np.int32, bleu_off=np.int32, ref_tok=np.int32, ref_off=np.int32,
        ref_len=np.int32, rimg_off=np.int32)
    want = S.brute_tables(corpus, end_idx)
    assert refs.n_images == len(want) == h["bleu_off"].shape[0] - 1 == h["rimg_off"].shape[0] - 1
    for k, (best, distinct) in enumerate(want):
        a, b = int(h["bleu_off"][k]), int(h["bleu_off"][k + 1])
        keys = h["bleu_keys"][a:b].tolist()
        assert keys == sorted(best) and h["bleu_cnt"][a:b].tolist() == [best[x] for x in keys], k
        r0, r1 = int(h["rimg_off"][k]), int(h["rimg_off"][k + 1])
        assert [h["ref_tok"][h["ref_off"][j]:h["ref_off"][j + 1]].tolist() for j in range(r0, r1)] == distinct, k
        assert h["ref_len"][r0:r1].tolist() == [len(d) for d in distinct]
    assert refs.n_keys == h["bleu_keys"].shape[0] and refs.n_tok == h["ref_tok"].shape[0]
    assert refs.n_refs == h["ref_len"].shape[0] == sum(len(d) for _, d in want)
    assert any(max(b.values() or [0]) > 1 for b, _ in want)  # a count above 1
    # the CIDEr-D tables are CiderRefs's, unchanged: every listed reference, repeats included
    plain = CiderRefs.build(corpus, end_idx=end_idx)
    assert plain.n_refs == sum(len(r) for r in corpus) > refs.n_refs
    for name, a in plain.host.items():
        assert np.array_equal(refs.cider.host[name], a), name
    assert refs.nbytes == sum(a.nbytes for a in h.values()) + plain.nbytes
    assert refs.bleu_keys.dtype.is_signed and refs.bleu_keys.shape[0] == refs.n_keys  # the bits travel as int64


def test_build_has_the_limits_of_cider_refs():
    from capmi.devscore import ScoreRefs
    ok = ScoreRefs.build([[[1] * 63]], end_idx=2)
    assert ok.host["ref_len"].tolist() == [64] and ok.end_idx == 2
    ScoreRefs.build([[[65533, 0]]])
    empty = ScoreRefs.build([[[]], [[], []]])  # no n-gram, no word
    assert empty.n_keys == 0 and empty.n_tok == 0 and empty.host["ref_len"].tolist() == [0, 0]
    assert empty.host["rimg_off"].tolist() == [0, 1, 2] and empty.host["bleu_off"].tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="63"):
        ScoreRefs.build([[[1] * 64]])
    with pytest.raises(ValueError, match="65533"):
        ScoreRefs.build([[[3, 65534]]])
    with pytest.raises(ValueError):
        ScoreRefs.build([[[3, -1]]])
    with pytest.raises(ValueError):
        ScoreRefs.build([[[3]], []])  # an image without a reference
    with pytest.raises(ValueError):
        ScoreRefs.build([])


def test_new_entry_points_are_declared_exported_and_bound():
    import capmi
    from capmi import kernels as K
    from capmi._lib import CAPMI_SCORE_STATS
    with open(os.path.join(REPO, "include", "capmi.h")) as f:
        text = f.read()
    assert int(re.search(r"#define CAPMI_SCORE_STATS (\d+)", text).group(1)) == CAPMI_SCORE_STATS == S.NS
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", text, flags=re.M), name
        assert hasattr(ctypes.CDLL(capmi.LIB_PATH), name)
        assert callable(getattr(K, name[len("capmi_"):])), name
    assert set(NEW) <= set(capmi.EXPORTS)
    assert capmi.ABI_VERSION == capmi.lib.capmi_abi_version() == 27


def _bad(fn, ok, **kw):
    a = list(ok)
    for pos, v in kw.items():
        a[int(pos[1:])] = v
    return fn(*a)


def test_entries_reject_bad_arguments_before_any_launch():
    """CAPMI_EINVAL / CAPMI_ERANGE: runs without a GPU."""
    import capmi
    lib = capmi.lib
    buf = (ctypes.c_float * 1024)()
    q = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    # tokens T R n lens img_key n_images V end score_end bleu_keys bleu_cnt n_keys bleu_off ref_tok n_tok ref_off
    # ref_len rimg_off stats bleu rouge stream
    ok = [q, 12, 6, 3, q, q, 5, 100, 2, 1, q, q, 7, q, q, 9, q, q, q, q, q, q, None]
    st = lambda **kw: _bad(lib.capmi_caption_stats, ok, **kw)  # noqa: E731
    for bad in (dict(p0=None), dict(p4=None), dict(p5=None), dict(p10=None), dict(p11=None), dict(p13=None),
                dict(p14=None), dict(p16=None), dict(p17=None), dict(p18=None), dict(p19=None), dict(p20=None),
                dict(p21=None), dict(p1=0), dict(p1=65), dict(p2=0), dict(p3=0), dict(p3=4), dict(p6=0), dict(p7=0),
                dict(p8=-1), dict(p12=-1), dict(p15=-1)):
        assert st(**bad) == EINVAL, bad
    assert st(p7=65535) == ERANGE
    assert st(p2=1 << 28, p3=1) == ERANGE  # R * CAPMI_SCORE_STATS past int32
    # cider bleu4 bleu_stride rouge R w_cider w_bleu4 w_rouge reward stream
    ok = [q, q, 4, q, 6, 1.0, 0.5, 0.0, q, None]
    mix = lambda **kw: _bad(lib.capmi_reward_mix, ok, **kw)  # noqa: E731
    for bad in (dict(p0=None), dict(p1=None), dict(p3=None), dict(p8=None), dict(p4=0), dict(p2=0),
                dict(p5=float("nan")), dict(p6=float("nan")), dict(p7=float("nan"))):
        assert mix(**bad) == EINVAL, bad
    assert mix(p2=1 << 40) == ERANGE


def _sum_rows(references, hypotheses):
    """corpus BLEU and ROUGE-L from the oracle's per-row integers, through capmi.devscore's fp64 formulas"""
    from capmi.devscore import bleu_from_counts, rouge_from_counts
    rows = np.array([S.row_integers(refs, hyp) for refs, hyp in zip(references, hypotheses)], dtype=np.int64)
    s = rows[:, :10].sum(axis=0).tolist()
    out = {f"Bleu_{k + 1}": b for k, b in enumerate(bleu_from_counts(s[0:4], s[4:8], s[8], s[9]))}
    out["ROUGE_L"] = sum(rouge_from_counts(*row) for row in rows[:, 10:14].tolist()) / len(rows)
    return out


@pytest.mark.parametrize("case", ["corpus", "single_image"])
def test_the_oracles_integers_reproduce_the_reference_scorers(golden, case):
    """The per-row integers, summed, give the fixture's corpus BLEU-1..4 and ROUGE-L at 1e-9 relative
    (tests/test_scoring_cpu.py's rule), and capmi.scoring's own numbers to the same bound."""
    from capmi.scoring import caption_scores
    c = golden[case]
    got = _sum_rows(c["references"], c["hypotheses"])
    host = caption_scores(c["references"], c["hypotheses"])
    for k, v in got.items():
        assert abs(v - c["scores"][k]) <= 1e-9 * abs(c["scores"][k]), (k, v, c["scores"][k])
        assert abs(v - host[k]) <= 1e-9 * abs(host[k]), (k, v, host[k])


def test_the_fixture_stays_inside_the_kernels_limits(golden):
    from capmi.scst import MAX_HYP_WORDS, MAX_REF_WORDS, MAX_TOKEN
    for c in golden.values():
        assert max(len(h) for h in c["hypotheses"]) <= MAX_HYP_WORDS
        assert max(len(r) for refs in c["references"] for r in refs) <= MAX_REF_WORDS
        assert 0 <= min(w for refs in c["references"] for r in refs for w in r)
        assert max([w for refs in c["references"] for r in refs for w in r]
                   + [w for h in c["hypotheses"] for w in h]) <= MAX_TOKEN


def test_the_oracles_rows_are_capmi_scoring_on_one_hypothesis(cases):
    """bleu / rouge of a row from its integers equal capmi.scoring.bleu / rouge_l on that row (1e-12 relative)."""
    from capmi.devscore import bleu_from_counts, rouge_from_counts
    for c in cases:
        stats, bleu, rouge = S.oracle(c)
        for r in range(c["R"]):
            if stats[r][0] < 0:
                continue
            s = stats[r].tolist()
            for a, b in zip(bleu_from_counts(s[0:4], s[4:8], s[8], s[9]), bleu[r]):
                assert abs(a - b) <= 1e-12 * abs(b)
            assert abs(rouge_from_counts(*s[10:14]) - rouge[r]) <= 1e-12 * abs(rouge[r])


def test_caption_scores_device_checks_its_arguments_like_the_host_scorer():
    from capmi.devscore import caption_scores_device
    for refs, hyps in (([[[1, 2]]], []), ([[[1, 2]], [[3]]], [[1]]), ([[]], [[1]])):
        with pytest.raises(ValueError):
            caption_scores_device(refs, hyps, "cuda")
    for refs, hyps in (([[[1] * 64]], [[1]]), ([[[1]]], [[1] * 65]), ([[[65534]]], [[1]]), ([[[1]]], [[-1]])):
        with pytest.raises(ValueError, match="caption_scores"):
            caption_scores_device(refs, hyps, "cuda")
    with pytest.raises(ValueError, match="caption_scores"):
        caption_scores_device([[[1, 2]]], [[1]], "cpu")


def test_cider_listing_keeps_the_mean_over_listed_references():
    from capmi.devscore import _cider_listing
    a, b = (1, 2), (3,)
    assert _cider_listing([a] * 24) == [a] and _cider_listing([a, b]) == [a, b]
    assert _cider_listing([a, b, a, b]) == [a, b]
    assert _cider_listing([a, a, b]) == [a, a, b]  # listed unequally often: the mean weighs a twice


def test_reward_mix_needs_score_refs_and_known_metrics():
    from capmi.devscore import ScoreRefs
    from capmi.scst import CiderRefs, _SelfCriticalStep
    plain, full = CiderRefs.build([[[1, 2, 3]]], end_idx=9), ScoreRefs.build([[[1, 2, 3]]], end_idx=9)
    assert _SelfCriticalStep._check_mix(None, plain) is None
    assert _SelfCriticalStep._check_mix(dict(cider=1.0, bleu4=0.5, rouge_l=0.0), full) == (1.0, 0.5, 0.0)
    assert _SelfCriticalStep._check_mix(dict(bleu4=2), full) == (0.0, 2.0, 0.0)
    for mix, refs in ((dict(cider=1.0), plain), (dict(meteor=1.0), full), ({}, full), ([1, 0, 0], full),
                      (dict(cider=float("nan")), full)):
        with pytest.raises(ValueError):
            _SelfCriticalStep._check_mix(mix, refs)


def test_eval_scorer_flag_defaults_to_host():
    import eval as E
    assert E.parse_args(["c.pth.tar", "--model_type", "attention"]).scorer == "host"
    assert E.parse_args(["c.pth.tar", "--model_type", "baseline", "--scorer", "device"]).scorer == "device"
    with pytest.raises(SystemExit):
        E.parse_args(["c.pth.tar", "--model_type", "attention", "--scorer", "gpu"])
