"""Helper of the caption-metric tests (not a test): seeded token tables with their reference corpora, and the fp64
oracle of capmi_caption_stats built on capmi.scoring (its n-gram counts, its LCS, its bleu and rouge_l on one
hypothesis at a time)."""
import random
from fractions import Fraction

import numpy as np

END = 2            # END of the corpora built with one
BIG = 65533        # the largest token a key holds
NS = 14            # CAPMI_SCORE_STATS


def _corpus(rng):
    """Images 0..: the edge cases by hand, then seeded ones. Words 3..40 besides the named ones (never END)."""
    word = lambda: rng.randint(3, 40)  # noqa: E731
    long63 = [word() for _ in range(63)]
    images = [
        [[5, 6, 7, 8]],                                          # 0: one reference
        [[word() for _ in range(rng.randint(1, 12))] for _ in range(16)],  # 1: sixteen references
        [long63],                                                # 2: 63 words (64 with END)
        [[], [5, 6]],                                            # 3: an empty reference
        [[0, BIG, 0, 7], [BIG, BIG]],                            # 4: tokens 0 and 65533
        [[9, 4, 9, 11]],                                         # 5: holds word 9 twice
        [[5, 6, 7, 8, 20, 21, 22, 23, 24, 25, 26, 27], [5, 6]],  # 6: best precision and best recall differ
        [[5, 6, 7, 8], [5, 6, 7, 8, 9, 10]],                     # 7: lengths 4 and 6 around a hypothesis of 5
        [[]],                                                    # 8: only an empty reference
        [[5, 6, 7], [5, 6, 7], [5, 6, 7, 8]],                    # 9: a repeated reference
    ]
    for _ in range(14):
        images.append([[word() for _ in range(rng.randint(2, 20))] for _ in range(rng.randint(1, 6))])
    return images, long63


def _noisy(rng, base, T):
    return [w if rng.random() < 0.7 else rng.randint(3, 40) for w in base if rng.random() < 0.9][:T]


def build_cases():
    """[{name, references (per image, END not appended), end_idx, T, n, score_end, hyps (R token lists as a rollout
    emits them: a final END where the row finished), img_key (R / n,; some lie off the table), R}]. Every case
    scores against the one corpus of ``_corpus``."""
    rng = random.Random(2024)
    images, long63 = _corpus(rng)
    n_img = len(images)
    by_hand = [  # (image, emitted tokens), T = 64
        (0, [5, 6, 7, 8, END]),                  # an exact copy
        (0, []),                                 # 0 words
        (0, [5]), (0, [5, 6]), (0, [5, 6, 7]),   # 1..3 words: no guess at the higher orders
        (0, [5, END]), (0, [9, 6, END]), (0, [5, 6, 9, END]),
        (2, long63 + [END]),                     # 64 words equal to the reference: bit 63 and the carry out of it
        (2, [long63[0]] * 64),                   # 64 words, unfinished
        (2, list(reversed(long63)) + [long63[0]]),
        (5, [9] * 64),                           # one word 64 times against a reference that holds it twice
        (6, [5, 6, 7, 8, END]),                  # lcs_p from the long reference, recall from the short one
        (7, [5, 6, 7, 8, 9]),                    # 5 words between references of 4 and 6 (5 and 7 with END)
        (7, [5, 6, 7, 8, END]),
        (7, [5, 6, 7, 8, 9, END]),               # 6 words with END between 5 and 7: the tie goes to 5
        (7, [5, 6, 7, 8, 9, 10, END]),           # the same tie once END is dropped
        (3, []), (3, [END]), (3, [5, 6, END]),   # an empty reference, an empty hypothesis
        (8, []), (8, [END]), (8, [7]),
        (4, [0, BIG, 0, 7, END]), (4, [BIG, BIG, BIG]), (4, [0]),
        (9, [5, 6, 7, END]), (9, [5, 6, 7, 8, END]),
        (1, images[1][3] + [END]),
        (n_img + 5, [5, 6, 7]),                  # off the table
        (-1, [5, 6, 7]),
    ]
    rows = list(by_hand)
    while len(rows) < 65:
        image = rng.randrange(n_img)
        hyp = _noisy(rng, rng.choice(images[image]), 63)
        rows.append((image, hyp + ([END] if rng.random() < 0.8 else [])))
    cases = []
    for score_end in (1, 0):
        cases.append(dict(name=f"edges_end{score_end}", references=images, end_idx=END, T=64, n=1,
                          score_end=score_end, hyps=[h for _, h in rows], img_key=[k for k, _ in rows]))
    # n = 5 samples per image, a short table, R = 65
    keys, hyps = [], []
    for g in range(13):
        image = n_img + 1 if g == 7 else rng.randrange(n_img)
        keys.append(image)
        for _ in range(5):
            base = rng.choice(images[image % n_img])
            hyp = _noisy(rng, base, 19)
            hyps.append(hyp + ([END] if rng.random() < 0.8 else []))
    cases.append(dict(name="n5", references=images, end_idx=END, T=20, n=5, score_end=1, hyps=hyps, img_key=keys))
    # one row, one step, tables without END
    cases.append(dict(name="t1_r1", references=images, end_idx=None, T=1, n=1, score_end=1, hyps=[[5]], img_key=[0]))
    cases.append(dict(name="t1_empty", references=images, end_idx=None, T=1, n=1, score_end=1, hyps=[[]],
                      img_key=[3]))
    # tables without END: a reference that is empty as scored
    rows = [(3, []), (3, [5, 6]), (3, [7]), (8, []), (8, [7]), (0, [5, 6, 7, 8]), (9, [5, 6, 7])]
    cases.append(dict(name="no_end", references=images, end_idx=None, T=8, n=1, score_end=1,
                      hyps=[h for _, h in rows], img_key=[k for k, _ in rows]))
    for c in cases:
        c["R"] = len(c["hyps"])
        assert c["R"] == len(c["img_key"]) * c["n"] and all(len(h) <= c["T"] for h in c["hyps"])
    return cases


def token_table(case):
    """(T, R) int32, -1 past a row's end, and lens (R,)"""
    tab = np.full((case["T"], case["R"]), -1, dtype=np.int32)
    lens = np.zeros(case["R"], dtype=np.int32)
    for r, h in enumerate(case["hyps"]):
        tab[:len(h), r] = h
        lens[r] = len(h)
    return tab, lens


def scored_references(case):
    """per image its references as scored: END appended when the case has one"""
    end = case["end_idx"]
    return [[list(r) + ([end] if end is not None else []) for r in refs] for refs in case["references"]]


def scored_hypothesis(case, hyp):
    """a row's words as scored: a final END dropped under score_end 0"""
    if not case["score_end"] and hyp and hyp[-1] == case["end_idx"]:
        return hyp[:-1]
    return list(hyp)


def row_integers(refs, hyp):
    """The CAPMI_SCORE_STATS integers of one hypothesis against one image's references, from capmi.scoring's
    counting: matches, guesses, lengths, lcs_p, (lcs_r, len_r) by the largest lcs / len_r (exact fractions; the
    shorter reference on equal ratios) and the hypothesis's length as ROUGE-L counts it."""
    from capmi.scoring import _distinct, _lcs, _ngrams
    refs = _distinct(refs)
    best = {}
    for ref in refs:
        for g, c in _ngrams(ref, 4).items():
            best[g] = max(best.get(g, 0), c)
    match = [0] * 4
    for g, c in _ngrams(hyp, 4).items():
        match[len(g) - 1] += min(c, best.get(g, 0))
    guess = [max(0, len(hyp) - k) for k in range(4)]
    closest = min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]
    empty = [None]
    h = list(hyp) or empty
    pairs = []
    for ref in refs:
        r = list(ref) or empty
        pairs.append((_lcs(r, h), len(r)))
    lcs_p = max(p[0] for p in pairs)
    lcs_r, len_r = min(pairs, key=lambda p: (-Fraction(p[0], p[1]), p[1]))
    return match + guess + [len(hyp), closest, lcs_p, lcs_r, len_r, len(h)]


def oracle(case):
    """(stats (R, NS) int64, bleu (R, 4) float64, rouge (R,) float64): -1 / NaN for a key off the table; bleu and
    rouge are capmi.scoring.bleu / rouge_l on that one hypothesis."""
    from capmi.scoring import bleu, rouge_l
    refs = scored_references(case)
    R, n = case["R"], case["n"]
    stats = np.full((R, NS), -1, dtype=np.int64)
    b = np.full((R, 4), np.nan)
    ro = np.full(R, np.nan)
    for r, hyp in enumerate(case["hyps"]):
        image = case["img_key"][r // n]
        if not 0 <= image < len(refs):
            continue
        hyp = scored_hypothesis(case, hyp)
        stats[r] = row_integers(refs[image], hyp)
        b[r] = bleu([refs[image]], [hyp])
        ro[r] = rouge_l([refs[image]], [hyp])
    return stats, b, ro


def ulps32(got, want64):
    """|got - fp32(want)| in units of the fp32 spacing at fp32(want); 0 where both are NaN"""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    d[both_nan] = 0.0
    d[np.isnan(d)] = np.inf
    return d


def brute_tables(references_by_image, end_idx=None):
    """The ScoreRefs tables by plain Python: per image {key: max count} and its distinct references."""
    from scst_cases import key_of
    from capmi.scoring import _ngrams
    out = []
    for refs in references_by_image:
        refs = [list(r) + ([end_idx] if end_idx is not None else []) for r in refs]
        distinct = [list(r) for r in dict.fromkeys(tuple(r) for r in refs)]
        best = {}
        for ref in distinct:
            for g, c in _ngrams(ref, 4).items():
                best[key_of(g)] = max(best.get(key_of(g), 0), c)
        out.append((best, distinct))
    return out


def mix64(weights, cider, bleu4, rouge):
    """the fp64 combination capmi_reward_mix evaluates, in its order"""
    wc, wb, wr = weights
    return (wc * np.asarray(cider, np.float64) + wb * np.asarray(bleu4, np.float64)) + wr * np.asarray(rouge, np.float64)



def check_coverage(cases):
    """Every shape and edge the kernel can go wrong at is in the cases."""
    assert {1, 64} <= {c["T"] for c in cases} and {1, 65} <= {c["R"] for c in cases}
    assert {1, 5} <= {c["n"] for c in cases} and {0, 1} <= {c["score_end"] for c in cases}
    seen = set()
    for c in cases:
        refs, (stats, _, rouge) = scored_references(c), oracle(c)
        for r, emitted in enumerate(c["hyps"]):
            image = c["img_key"][r // c["n"]]
            if not 0 <= image < len(refs):
                seen.add("key off the table")
                assert (stats[r] == -1).all() and np.isnan(rouge[r])
                continue
            hyp, rs = scored_hypothesis(c, emitted), refs[image]
            seen.add(f"{min(len(hyp), 4) if len(hyp) < 64 else 64} words")
            if len(emitted) < c["T"]:
                seen.add("lens < T")
            if len(hyp) < len(emitted):
                seen.add("END dropped")
            seen.add(f"{len(rs)} references")
            if any(len(x) == 64 for x in rs) and c["end_idx"] is not None:
                seen.add("63 words plus END")
            if any(len(x) == 0 for x in rs):
                seen.add("empty reference")
                if not hyp:
                    seen.add("empty against empty")
                    assert stats[r][10] == 1 and rouge[r] > 0
            if {0, BIG} <= set(hyp) and {0, BIG} <= {w for x in rs for w in x}:
                seen.add("tokens 0 and 65533")
            if len(hyp) == 64 and len(set(hyp)) == 1 and stats[r][0] == 2:
                seen.add("clipped 64 to 2")
            if len(hyp) == 64 and stats[r][10] == 64:
                seen.add("LCS 64")
            if stats[r][10] > stats[r][11] > 0:
                seen.add("precision and recall from different references")
            d = sorted({(abs(len(x) - len(hyp)), len(x)) for x in rs})
            if len(d) > 1 and d[0][0] == d[1][0]:
                seen.add("length tie")
                assert stats[r][9] == d[0][1] < d[1][1]
            if rouge[r] == 0:
                seen.add("ROUGE 0")
    want = {"key off the table", "0 words", "1 words", "2 words", "3 words", "64 words", "lens < T", "END dropped",
            "1 references", "16 references", "63 words plus END", "empty reference", "empty against empty",
            "tokens 0 and 65533", "clipped 64 to 2", "LCS 64", "precision and recall from different references",
            "length tie", "ROUGE 0"}
    assert want <= seen, sorted(want - seen)
