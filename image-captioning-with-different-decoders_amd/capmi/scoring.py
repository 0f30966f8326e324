"""Caption scoring on the CPU: corpus BLEU-1..4, ROUGE-L and CIDEr over token-id captions.

Written from the published definitions (Papineni et al. 2002; Lin 2004; Vedantam et al. 2015) with the
conventions of the COCO caption evaluation the reference project scores with, so the numbers are
comparable with its eval.py:

* BLEU: corpus level (n-gram matches and lengths summed over images before the ratio), hypothesis counts
  clipped by the maximum count over the image's references, brevity penalty against the reference length
  closest to the hypothesis (the shorter on a tie), and the additive constants ``tiny`` / ``small`` that keep
  an empty hypothesis at 0 instead of 0/0.
* ROUGE-L: F-measure with beta = 1.2 of the best LCS precision and the best LCS recall over the image's
  references, averaged over images. An empty sentence counts as one empty token (what splitting an empty
  string on a blank gives), so it has length 1 and matches only another empty sentence.
* CIDEr: n = 1..4 TF-IDF vectors, document frequency = number of images whose reference set holds the
  n-gram, IDF = log(#images) - log(max(1, df)) (with a single image the log(#images) term is taken as 1),
  clipped cosine similarity, Gaussian length penalty with sigma = 6 on the difference of the sentences'
  bigram counts, mean over n and over the references, times 10, averaged over images.

METEOR is not computed (it needs an external Java tool): the key is absent from the result.
"""
import math
from collections import Counter

BLEU_N = 4
BLEU_TINY = 1e-15
BLEU_SMALL = 1e-9
ROUGE_BETA = 1.2
CIDER_N = 4
CIDER_SIGMA = 6.0


def _ngrams(tokens, n):
    """Counts of the 1..n-grams of a token sequence, keyed by tuple."""
    tokens = tuple(tokens)
    c = {}
    for k in range(1, n + 1):
        for i in range(len(tokens) - k + 1):
            g = tokens[i:i + k]
            c[g] = c.get(g, 0) + 1
    return c


def _distinct(refs):
    """An image's distinct references. The validation pass repeats one target once per target position
    (models.attention.evaluate_batched), and a maximum over references needs each only once."""
    return list(dict.fromkeys(tuple(r) for r in refs))


def bleu(references, hypotheses, n=BLEU_N):
    """Corpus BLEU-1..n: list of n floats."""
    correct, guess = [0] * n, [0] * n
    hyp_len = ref_len = 0
    for refs, hyp in zip(references, hypotheses):
        refs = _distinct(refs)
        hc = _ngrams(hyp, n)
        best = {}
        for ref in refs:
            for g, c in _ngrams(ref, n).items():
                if c > best.get(g, 0):
                    best[g] = c
        for g, c in hc.items():
            correct[len(g) - 1] += min(c, best.get(g, 0))
        for k in range(n):
            guess[k] += max(0, len(hyp) - k)
        hyp_len += len(hyp)
        ref_len += min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]
    out, prod = [], 1.0
    for k in range(n):
        prod *= (correct[k] + BLEU_TINY) / (guess[k] + BLEU_SMALL)
        out.append(prod ** (1.0 / (k + 1)))
    ratio = (hyp_len + BLEU_TINY) / (ref_len + BLEU_SMALL)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


def _lcs(a, b):
    """Length of the longest common subsequence."""
    if len(a) < len(b):
        a, b = b, a
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b, 1):
            cur.append(prev[j - 1] + 1 if x == y else max(prev[j], cur[j - 1]))
        prev = cur
    return prev[len(b)]


def rouge_l(references, hypotheses, beta=ROUGE_BETA):
    """Mean over images of the ROUGE-L F-measure."""
    empty = [None]  # the one token of an empty sentence
    scores = []
    for refs, hyp in zip(references, hypotheses):
        h = list(hyp) or empty
        prec = rec = 0.0
        for ref in _distinct(refs):
            r = list(ref) or empty
            lcs = _lcs(r, h)
            prec = max(prec, lcs / float(len(h)))
            rec = max(rec, lcs / float(len(r)))
        if prec != 0 and rec != 0:
            scores.append(((1 + beta ** 2) * prec * rec) / float(rec + beta ** 2 * prec))
        else:
            scores.append(0.0)
    return math.fsum(scores) / len(scores)


def cider(references, hypotheses, n=CIDER_N, sigma=CIDER_SIGMA):
    """Mean over images of the CIDEr score."""
    # per image: its distinct references' n-gram counts, and which of them each listed reference is (a
    # repeated reference is scored once and added once per listing, as the mean over references needs)
    ref_counts, ref_index = [], []
    for refs in references:
        distinct = _distinct(refs)
        where = {r: i for i, r in enumerate(distinct)}
        ref_counts.append([_ngrams(r, n) for r in distinct])
        ref_index.append([where[tuple(r)] for r in refs])
    df = Counter()
    for counts in ref_counts:
        df.update(set(g for c in counts for g in c))
    log_images = math.log(float(len(ref_counts))) if len(ref_counts) != 1 else 1.0

    def tfidf(counts):
        vec = [{} for _ in range(n)]
        norm = [0.0] * n
        bigrams = 0
        for g, tf in counts.items():
            k = len(g) - 1
            w = float(tf) * (log_images - math.log(max(1.0, float(df.get(g, 0)))))
            vec[k][g] = w
            norm[k] += w * w
            if k == 1:
                bigrams += tf
        return vec, [math.sqrt(x) for x in norm], bigrams

    scores = []
    for counts, index, hyp in zip(ref_counts, ref_index, hypotheses):
        hv, hn, hl = tfidf(_ngrams(hyp, n))
        sims = []
        for rc in counts:
            rv, rn, rl = tfidf(rc)
            penalty = math.e ** (-(float(hl - rl) ** 2) / (2 * sigma ** 2))
            sim = []
            for k in range(n):
                val = 0.0
                for g, w in hv[k].items():
                    wr = rv[k].get(g, 0.0)
                    val += min(w, wr) * wr
                if hn[k] != 0 and rn[k] != 0:
                    val /= hn[k] * rn[k]
                sim.append(val * penalty)
            sims.append(sim)
        total = [0.0] * n
        for i in index:
            for k in range(n):
                total[k] += sims[i][k]
        scores.append(math.fsum(total) / n / len(index) * 10.0)
    return math.fsum(scores) / len(scores)


def caption_scores(references, hypotheses):
    """references: per image a list of reference captions (token-id lists); hypotheses: per image one
    caption (token-id list) -- the nested lists the reference's ``get_eval_score`` takes.
    Returns {"Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"} as Python floats."""
    if len(references) != len(hypotheses) or not hypotheses:
        raise ValueError("caption_scores needs as many reference sets as hypotheses, and at least one")
    if any(len(refs) == 0 for refs in references):
        raise ValueError("every image needs at least one reference caption")
    out = {f"Bleu_{k + 1}": float(b) for k, b in enumerate(bleu(references, hypotheses))}
    out["ROUGE_L"] = float(rouge_l(references, hypotheses))
    out["CIDEr"] = float(cider(references, hypotheses))
    return out
