"""Writes tests/golden/caption_scores.json: seeded token-id captions and the scores the reference
project's scorers give them.

    python tests/golden/make_scores_golden.py /path/to/Image-Captioning-with-Different-Decoders

The scorers are called as the reference's metric.get_eval_score calls them (token ids joined into blank-
separated strings, one hypothesis and a list of references per image), without METEOR (it needs a Java
tool). Needs the reference checkout; the committed fixture is what the tests read.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def make_inputs(seed=20261019, n_random=30, vocab=40):
    """references / hypotheses in evaluate()'s shape: per image the stripped target repeated once per
    target position (the reference's quirk), and one hypothesis."""
    rng = random.Random(seed)
    refs, hyps = [], []

    def add(target, hyp, repeats=None):
        # target positions of START w1..wn END teacher-forced: w1..wn END = n + 1
        refs.append([list(target) for _ in range(len(target) + 1 if repeats is None else repeats)])
        hyps.append(list(hyp))

    for _ in range(n_random):
        n = rng.randint(3, 14)
        target = [rng.randint(1, vocab) for _ in range(n)]
        hyp = []
        for w in target:  # a noisy copy: substitutions, drops and insertions
            u = rng.random()
            if u < 0.55:
                hyp.append(w)
            elif u < 0.75:
                hyp.append(rng.randint(1, vocab))
            elif u < 0.85:
                hyp.extend([w, rng.randint(1, vocab)])
        add(target, hyp)
    add([5, 6, 7, 8, 9, 10], [5, 6, 7, 8, 9, 10])          # exact match
    add([11, 12, 13, 14, 15], [11, 12, 13])                # hypothesis shorter than 4 tokens
    add([3, 4, 5, 6], [4])                                 # a single token
    add([21, 22, 23, 24, 25, 26, 27], [])                  # empty hypothesis
    add([1, 2, 3, 4, 5], [31, 32, 33, 34, 35, 36])         # nothing in common
    add([7, 7, 7, 8, 8], [7, 7, 7, 7, 7, 7, 8])            # repeated words: clipping
    add([9, 10, 11, 12, 13, 14, 15, 16], [9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20])  # much longer
    # several different references for one image: closest-length and max-over-references paths
    refs.append([[1, 2, 3, 4, 5, 6], [1, 2, 3, 9], [2, 3, 4, 5, 6, 7, 8, 9, 10]])
    hyps.append([1, 2, 3, 4, 9])
    refs.append([[12, 13, 14], [12, 13, 14, 15, 16, 17, 18]])  # two references equally far in length
    hyps.append([12, 13, 14, 15, 16])
    return refs, hyps


def reference_scores(root, references, hypotheses):
    sys.path.insert(0, root)
    from eval_func.bleu.bleu import Bleu
    from eval_func.cider.cider import Cider
    from eval_func.rouge.rouge import Rouge
    hypo = [[' '.join(str(x) for x in h)] for h in hypotheses]
    ref = [[' '.join(str(x) for x in r) for r in rs] for rs in references]
    out = {}
    for scorer, names in ((Bleu(4), ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4"]), (Rouge(), "ROUGE_L"),
                          (Cider(), "CIDEr")):
        score, _ = scorer.compute_score(ref, hypo)
        if isinstance(names, list):
            out.update({k: float(v) for k, v in zip(names, score)})
        else:
            out[names] = float(score)
    return out


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    cases = {}
    refs, hyps = make_inputs()
    cases["corpus"] = {"references": refs, "hypotheses": hyps}
    cases["single_image"] = {"references": refs[3:4], "hypotheses": hyps[3:4]}
    for c in cases.values():
        c["scores"] = reference_scores(argv[1], c["references"], c["hypotheses"])
    with open(os.path.join(HERE, "caption_scores.json"), "w") as f:
        json.dump(cases, f, indent=None, separators=(",", ":"))
        f.write("\n")
    for name, c in cases.items():
        print(name, len(c["hypotheses"]), c["scores"])


if __name__ == "__main__":
    main(sys.argv)
