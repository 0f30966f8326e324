"""Caption metrics on the device: BLEU-1..4, ROUGE-L and CIDEr-D of token-id captions on the capmi kernels.

``ScoreRefs``             the reference tables ``capmi_caption_stats`` reads, next to the ``CiderRefs`` of the same
                          captions (``.cider``): per image the clipping counts of BLEU and the distinct references of
                          ROUGE-L
``DeviceCaptionScorer``   one (T, R) token table -> per-row integers, sentence-level BLEU / ROUGE-L and CIDEr-D, all
                          device tensors (a self-critical step mixes them: capmi.scst, ``reward_mix``)
``corpus_scores_from_rows`` the corpus formulas on per-image rows gathered from any number of ``score_table`` calls
                          (capmi.genval scores batch by batch)
``caption_scores_device`` capmi.scoring.caption_scores with the counting on the device: the corpus scores of the
                          validation pass from the rows' integers, finished in fp64 with capmi.scoring's formulas

Limits (those of the n-gram keys and of one lane per word): a hypothesis of at most 64 words, a reference of at most
63 (64 with its END), tokens 0..65533.
"""
import math

import numpy as np
import torch

from . import kernels as K
from ._lib import CAPMI_SCORE_STATS
from .scoring import BLEU_N, BLEU_SMALL, BLEU_TINY, ROUGE_BETA
from .scst import MAX_HYP_WORDS, MAX_REF_WORDS, MAX_TOKEN, CiderRefs, _flat_keys

# columns of a stats row (capmi_caption_stats in capmi.h)
MATCH, GUESS, HYP_LEN, REF_LEN, LCS_P, LCS_R, LEN_R, ROUGE_HYP_LEN = 0, 4, 8, 9, 10, 11, 12, 13
METRICS = ("cider", "bleu4", "rouge_l")


class ScoreRefs:
    """The references of BLEU, ROUGE-L and CIDEr-D as tables on ``device`` (layouts: capmi_caption_stats in
    capmi.h). ``cider`` is the ``CiderRefs`` of the same captions; host copies of the new tables stay in ``host``
    (numpy)."""

    @classmethod
    def build(cls, references_by_image, end_idx=None, device="cpu"):
        """references_by_image, end_idx: as ``CiderRefs.build`` takes them (same limits, same ``ValueError``s)."""
        self = cls()
        self.cider = CiderRefs.build(references_by_image, end_idx=end_idx, device=device)
        self.end_idx, self.n_images = self.cider.end_idx, self.cider.n_images
        # BLEU clips by the maximum over references and ROUGE-L keeps the best one: a repeated reference changes
        # nothing (the validation pass lists one reference once per target position)
        distinct = [list(dict.fromkeys(tuple(r) for r in caps)) for caps in self.cider.references]  # END appended
        self.references = distinct
        refs = [r for caps in distinct for r in caps]
        per_image = np.array([len(caps) for caps in distinct], dtype=np.int64)
        n_refs = len(refs)
        img_of_ref = np.repeat(np.arange(self.n_images, dtype=np.int64), per_image)
        lens = np.array([len(r) for r in refs], dtype=np.int64)
        tokens = np.array([w for r in refs for w in r], dtype=np.int64)
        rid = np.repeat(np.arange(n_refs, dtype=np.int64), lens)
        keys, owner = _flat_keys(tokens.astype(np.uint64) + np.uint64(1), rid)
        # count per (reference, key), then per (image, key) the largest count: sorted by image, key, count, the
        # last entry of every (image, key) run
        order = np.lexsort((keys, owner))
        keys, owner = keys[order], owner[order]
        new = np.ones(keys.shape[0], dtype=bool)
        new[1:] = (keys[1:] != keys[:-1]) | (owner[1:] != owner[:-1])
        starts = np.flatnonzero(new)
        tf = np.diff(np.append(starts, keys.shape[0]))
        ekeys, eimg = keys[starts], img_of_ref[owner[starts]]
        o2 = np.lexsort((tf, ekeys, eimg))
        ekeys, eimg, tf = ekeys[o2], eimg[o2], tf[o2]
        last = np.ones(ekeys.shape[0], dtype=bool)
        last[:-1] = (ekeys[1:] != ekeys[:-1]) | (eimg[1:] != eimg[:-1])
        bleu_keys, bleu_img, bleu_cnt = ekeys[last], eimg[last], tf[last]
        if max(bleu_keys.shape[0], tokens.shape[0]) >= 2 ** 31 - 1:
            raise ValueError("the reference tables are indexed with int32")
        self.n_refs, self.n_keys, self.n_tok = n_refs, int(bleu_keys.shape[0]), int(tokens.shape[0])
        csr = lambda counts: np.concatenate(([0], np.cumsum(counts))).astype(np.int32)  # noqa: E731
        self.host = dict(
            bleu_keys=bleu_keys, bleu_cnt=bleu_cnt.astype(np.int32),
            bleu_off=csr(np.bincount(bleu_img, minlength=self.n_images)),
            ref_tok=tokens.astype(np.int32), ref_off=csr(lens), ref_len=lens.astype(np.int32),
            rimg_off=csr(per_image))
        return self.to(device)

    def to(self, device):
        self.device = torch.device(device)
        if self.cider.device != self.device:
            self.cider.to(device)
        for name, a in self.host.items():
            if a.dtype == np.uint64:  # torch has no uint64 arithmetic: the bits travel as int64
                a = a.view(np.int64)
            setattr(self, name, torch.from_numpy(np.ascontiguousarray(a)).to(self.device))
        return self

    @property
    def nbytes(self):
        """Bytes of device memory the tables take, the CIDEr-D tables included."""
        return int(sum(a.nbytes for a in self.host.values())) + self.cider.nbytes


class DeviceCaptionScorer:
    """Scores token tables against ``refs`` (a ``ScoreRefs`` on a HIP device)."""

    def __init__(self, refs):
        if not isinstance(refs, ScoreRefs):
            raise ValueError("DeviceCaptionScorer needs a ScoreRefs")
        self.refs = refs

    def score_table(self, tokens, lens, img_key, n=1, score_end=True):
        """tokens (T, R) int32, lens (R,), img_key (R / n,): the sampler's layout (row r belongs to image
        img_key[r // n]). ``score_end`` False drops a final END (needs tables built with ``end_idx``). Returns
        {"stats" (R, CAPMI_SCORE_STATS) int32, "bleu" (R, 4), "rouge" (R,), "cider" (R,)} on the device."""
        refs = self.refs
        T, R = tokens.shape
        if not score_end and refs.end_idx is None:
            raise ValueError("score_end=False needs tables built with end_idx")
        end = 0 if refs.end_idx is None else refs.end_idx
        dev = tokens.device
        out = dict(stats=torch.empty(R, CAPMI_SCORE_STATS, dtype=torch.int32, device=dev),
                   bleu=torch.empty(R, 4, dtype=torch.float32, device=dev),
                   rouge=torch.empty(R, dtype=torch.float32, device=dev),
                   cider=torch.empty(R, dtype=torch.float32, device=dev))
        K.cider_reward(tokens, T, R, n, lens, img_key, refs.cider, MAX_TOKEN + 1, end, score_end, out["cider"])
        K.caption_stats(tokens, T, R, n, lens, img_key, refs, MAX_TOKEN + 1, end, score_end, out["stats"],
                        out["bleu"], out["rouge"])
        return out

    def corpus_scores(self, hypotheses):
        """The six corpus scores of ``capmi.scoring.caption_scores`` for one hypothesis per image of the tables, in
        image order: one (T, R) table, one launch of each kernel, BLEU from the ten summed integers and ROUGE-L
        from the rows' integers in fp64 on the host, CIDEr the fp64 mean of the rows' fp32 rewards."""
        refs = self.refs
        R = len(hypotheses)
        if R != refs.n_images:
            raise ValueError("one hypothesis per image of the tables")
        T = max(1, max(len(h) for h in hypotheses))
        table = np.full((T, R), -1, dtype=np.int32)
        lens = np.zeros(R, dtype=np.int32)
        for r, h in enumerate(hypotheses):
            table[:len(h), r] = h
            lens[r] = len(h)
        dev = lambda a: torch.from_numpy(a).to(refs.device)  # noqa: E731
        out = self.score_table(dev(table), dev(lens), dev(np.arange(R, dtype=np.int32)))
        return corpus_scores_from_rows(out["stats"].cpu().numpy(), out["cider"].cpu().numpy())


def corpus_scores_from_rows(stats, cider):
    """The six corpus scores from the rows ``score_table`` gives, one row per image: ``stats`` (N,
    CAPMI_SCORE_STATS) integers, ``cider`` (N,) floats, on the host. BLEU from the ten summed integers and ROUGE-L
    from the rows' integers in fp64, CIDEr the fp64 mean of the rows' rewards. A pass that scores batch by batch
    gathers its rows into one table and calls this once."""
    stats = np.asarray(stats).astype(np.int64)
    cider = np.asarray(cider).astype(np.float64)
    R = stats.shape[0]
    if stats.ndim != 2 or stats.shape[1] != CAPMI_SCORE_STATS or cider.shape != (R,) or R < 1:
        raise ValueError("corpus_scores_from_rows takes (N, CAPMI_SCORE_STATS) integers and (N,) floats, N >= 1")
    s = stats[:, :REF_LEN + 1].sum(axis=0).tolist()
    scores = {f"Bleu_{k + 1}": float(b) for k, b in enumerate(
        bleu_from_counts(s[MATCH:MATCH + 4], s[GUESS:GUESS + 4], s[HYP_LEN], s[REF_LEN]))}
    rows = stats[:, [LCS_P, LCS_R, LEN_R, ROUGE_HYP_LEN]].tolist()
    scores["ROUGE_L"] = float(math.fsum(rouge_from_counts(*row) for row in rows) / R)
    scores["CIDEr"] = float(math.fsum(cider.tolist()) / R)
    return scores


def bleu_from_counts(correct, guess, hyp_len, ref_len):
    """capmi.scoring.bleu from its summed integers: BLEU-1..4."""
    out, prod = [], 1.0
    for k in range(BLEU_N):
        prod *= (correct[k] + BLEU_TINY) / (guess[k] + BLEU_SMALL)
        out.append(prod ** (1.0 / (k + 1)))
    ratio = (hyp_len + BLEU_TINY) / (ref_len + BLEU_SMALL)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


def rouge_from_counts(lcs_p, lcs_r, len_r, hyp_len, beta=ROUGE_BETA):
    """capmi.scoring.rouge_l's F-measure of one image from its integers (``hyp_len`` as ROUGE-L counts it)."""
    prec, rec = lcs_p / float(hyp_len), lcs_r / float(len_r)
    if prec != 0 and rec != 0:
        return ((1 + beta ** 2) * prec * rec) / float(rec + beta ** 2 * prec)
    return 0.0


def _cider_listing(refs):
    """An image's references as the CIDEr-D table lists them. The mean over the listed references equals the mean
    over the distinct ones when every distinct reference is listed equally often (the validation pass's one
    repeated reference, COCO's five distinct ones): then the distinct ones, else the listing as given."""
    counts = {}
    for r in refs:
        counts[r] = counts.get(r, 0) + 1
    return list(counts) if len(set(counts.values())) == 1 else refs


def caption_scores_device(references, hypotheses, device):
    """``capmi.scoring.caption_scores(references, hypotheses)`` with the n-gram counting, the LCS and the CIDEr-D
    rows on ``device``: one (T, R) table, one launch of each kernel, the corpus formulas in fp64 on the host.
    Same arguments, keys and ``ValueError``s; a caption outside the kernels' limits is a ``ValueError`` too."""
    if len(references) != len(hypotheses) or not hypotheses:
        raise ValueError("caption_scores needs as many reference sets as hypotheses, and at least one")
    if any(len(refs) == 0 for refs in references):
        raise ValueError("every image needs at least one reference caption")
    if torch.device(device).type != "cuda":
        raise ValueError("caption_scores_device needs a HIP device; capmi.scoring.caption_scores scores on the host")
    hyps = [[int(w) for w in h] for h in hypotheses]
    # the tables' listing holds every distinct reference: the limits are checked on it, not on every repeat
    listed = [_cider_listing([tuple(r) for r in refs]) for refs in references]
    fits = lambda c, words: len(c) <= words and (not c or (min(c) >= 0 and max(c) <= MAX_TOKEN))  # noqa: E731
    if not (all(fits(h, MAX_HYP_WORDS) for h in hyps)
            and all(fits(r, MAX_REF_WORDS) for refs in listed for r in refs)):
        raise ValueError(f"caption_scores_device takes hypotheses of at most {MAX_HYP_WORDS} words, references of "
                         f"at most {MAX_REF_WORDS} and tokens 0..{MAX_TOKEN}: use capmi.scoring.caption_scores")
    refs = ScoreRefs.build(listed, device=device)
    return DeviceCaptionScorer(refs).corpus_scores(hyps)
