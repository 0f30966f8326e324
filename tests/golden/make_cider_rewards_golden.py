"""Writes tests/golden/cider_rewards.json: a seeded corpus of token-id references, hypotheses per image and the
per-image CIDEr the reference project's CiderScorer gives each of them.

    python tests/golden/make_cider_rewards_golden.py /path/to/Image-Captioning-with-Different-Decoders

Every image has the same HYPS_PER_IMAGE kinds of hypothesis (see ``image``); sample index j of every image is one
scorer run, so the document frequencies are the whole corpus's, as in self-critical training. Each run is made
twice: on the plain words ("scores"), and with END appended to every reference and to every finished hypothesis
("scores_end"). Needs the reference checkout; the committed fixture is what the tests read.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
END = 65000       # no other word of the corpus
COMMON = 1        # the first word of every reference: df = the number of images, idf 0
HYPS_PER_IMAGE = 9


def noisy(rng, target, vocab):
    """make_scores_golden.make_inputs' noisy copy: substitutions, drops and insertions"""
    hyp = []
    for w in target:
        u = rng.random()
        if u < 0.55:
            hyp.append(w)
        elif u < 0.75:
            hyp.append(rng.randint(2, vocab))
        elif u < 0.85:
            hyp.extend([w, rng.randint(2, vocab)])
    return hyp


def image(refs, first, first_finished=(True, True, True)):
    """An image's references and its hypotheses: three of its own (noisy copies, or hand-made), the empty one
    unfinished and finished (END alone), the first 1, 2, 3 words of reference 0 (the first unfinished), and
    reference 0 itself."""
    r0 = refs[0]
    hyps = [list(h) for h in first] + [[], [], r0[:1], r0[:2], r0[:3], list(r0)]
    fin = list(first_finished) + [False, True, False, True, True, True]
    assert len(hyps) == len(fin) == HYPS_PER_IMAGE
    assert all(len(h) + f <= 64 for h, f in zip(hyps, fin))
    return {"references": [list(r) for r in refs], "hyps": hyps, "finished": fin}


def make_corpus(seed=20261021, n_random=32, vocab=40):
    rng = random.Random(seed)
    images = []
    for _ in range(n_random):
        refs = []
        for _ in range(rng.randint(1, 7)):
            if refs and rng.random() < 0.2:
                refs.append(list(rng.choice(refs)))  # a reference listed twice
            else:
                refs.append([COMMON] + [rng.randint(2, vocab) for _ in range(rng.randint(3, 14))])
        images.append(image(refs, [noisy(rng, rng.choice(refs), vocab) for _ in range(3)]))
    # one reference; an exact copy, a permutation and a 4-gram-free overlap
    images.append(image([[COMMON, 5, 6, 7, 8, 9, 10]], [[COMMON, 5, 6, 7, 8, 9, 10], [10, 9, 8, 7, 6, 5, COMMON],
                                                        [5, 6, 7, 20, 8, 9, 10]]))
    # seven references
    images.append(image([[COMMON] + [rng.randint(2, vocab) for _ in range(4 + j)] for j in range(7)],
                        [[COMMON, 2, 3], [COMMON] + [rng.randint(2, vocab) for _ in range(9)], [COMMON]]))
    # repeated words: tf > 1 and clipping
    images.append(image([[COMMON, 7, 7, 7, 8, 8], [COMMON, 7, 8, 7, 8]],
                        [[7, 7, 7, 7, 7, 7, 8], [COMMON, 7, 7, 7, 8, 8, 8, 8], [8, 8, 7, 7]]))
    # no word in common; n-grams found in no reference at all (words 50..56: df 0)
    images.append(image([[COMMON, 2, 3, 4, 5]], [[31, 32, 33, 34, 35, 36], [50, 51, 52, 53, 54, 55, 56],
                                                 [COMMON, 2, 50, 51, 3, 4, 5]]))
    # token ids 0 and 65533
    images.append(image([[COMMON, 0, 65533, 5, 0], [0, 0, 65533, 65533]],
                        [[0, 65533, 5, 0, 65533], [COMMON, 0, 65533, 5, 0], [65533, 0]]))
    # a hypothesis of 64 words without END against a reference of 63
    long_ref = [COMMON] + [rng.randint(2, vocab) for _ in range(62)]
    images.append(image([long_ref, long_ref[:20]], [long_ref + [9], long_ref[:40] + long_ref[:24], long_ref[1:]],
                        (False, False, True)))
    return images


def scorer_runs(root, images):
    """scores[image][j] from one CiderScorer run per sample index j; plain and with END"""
    sys.path.insert(0, root)
    from eval_func.cider.cider_scorer import CiderScorer
    words = lambda toks: ' '.join(str(x) for x in toks)  # noqa: E731
    out = {}
    for name, with_end in (("scores", False), ("scores_end", True)):
        per_image = [[] for _ in images]
        for j in range(HYPS_PER_IMAGE):
            cs = CiderScorer(n=4, sigma=6.0)
            for im in images:
                hyp = im["hyps"][j] + ([END] if with_end and im["finished"][j] else [])
                cs += (words(hyp), [words(r + ([END] if with_end else [])) for r in im["references"]])
            _, scores = cs.compute_score()
            for k, s in enumerate(scores):
                per_image[k].append(float(s))
        out[name] = per_image
    return out


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    corpus = make_corpus()
    cases = {"corpus": corpus, "single_image": corpus[32:33]}
    doc = {"end_idx": END, "hyps_per_image": HYPS_PER_IMAGE}
    for name, images in cases.items():
        doc[name] = {"images": images, **scorer_runs(argv[1], images)}
    with open(os.path.join(HERE, "cider_rewards.json"), "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    for name in cases:
        flat = [s for per in doc[name]["scores"] for s in per]
        print(name, len(doc[name]["images"]), "images", len(flat), "scores", "max", max(flat),
              "zeros", sum(s == 0 for s in flat))


if __name__ == "__main__":
    main(sys.argv)
