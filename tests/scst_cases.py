"""Helper of the self-critical training tests (not a test): the CIDEr reward fixture as rows, the token table a
batch of rows makes, and the reward formula restated in numpy float32 with sequential sums (the measure of what
fp32 arithmetic costs, from which tests/test_gpu_scst.py takes the kernel's bound)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
ULP_AT_10 = 9.5e-7  # one fp32 ulp of a reward near its maximum of 10


def load_fixture():
    with open(os.path.join(HERE, "golden", "cider_rewards.json")) as f:
        return json.load(f)


def case_rows(case):
    """Every (image, hypothesis) of a fixture case: dicts with image, j, hyp, finished, score, score_end."""
    rows = []
    for i, im in enumerate(case["images"]):
        for j, (h, fin) in enumerate(zip(im["hyps"], im["finished"])):
            rows.append(dict(image=i, j=j, hyp=h, finished=fin, score=case["scores"][i][j],
                             score_end=case["scores_end"][i][j]))
    return rows


def references(case):
    return [im["references"] for im in case["images"]]


def emitted(row, end_idx):
    """the tokens a rollout of this hypothesis leaves in its column of the table"""
    return row["hyp"] + ([end_idx] if row["finished"] else [])


def token_table(rows, T, end_idx):
    """(T, R) int32 table, -1 past a row's end, and lens (R,)"""
    tab = np.full((T, len(rows)), -1, dtype=np.int32)
    lens = np.zeros(len(rows), dtype=np.int32)
    for r, row in enumerate(rows):
        e = emitted(row, end_idx)
        assert len(e) <= T
        tab[:len(e), r] = e
        lens[r] = len(e)
    return tab, lens


def key_of(gram):
    k = 0
    for j, w in enumerate(gram):
        k |= (int(w) + 1) << (48 - 16 * j)
    return k


def reward_f32(refs, hyp, image):
    """The reward of one hypothesis (END already kept or dropped) against image ``image`` of the CiderRefs
    ``refs``, every operation in numpy float32 on the fp32 tables, sums in key order (dict insertion order of the
    hypothesis for the products, as the scorers')."""
    h = refs.host
    idf = refs.__dict__.get("_idf_by_key")
    if idf is None:
        idf = refs.__dict__["_idf_by_key"] = dict(zip(h["idf_keys"].tolist(), h["idf_vals"]))
    counts = [{} for _ in range(4)]
    for n in range(1, 5):
        for i in range(len(hyp) - n + 1):
            k = key_of(hyp[i:i + n])
            counts[n - 1][k] = counts[n - 1].get(k, 0) + 1
    wh = [{k: F32(tf) * idf.get(k, F32(refs.log_images)) for k, tf in c.items()} for c in counts]
    hn = []
    for n in range(4):
        s = F32(0)
        for w in wh[n].values():
            s = F32(s + F32(w * w))
        hn.append(np.sqrt(s))
    hl = max(len(hyp) - 1, 0)
    score = [F32(0)] * 4
    r0, r1 = int(h["img_off"][image]), int(h["img_off"][image + 1])
    for ref in range(r0, r1):
        e0, e1 = int(h["ref_off"][ref]), int(h["ref_off"][ref + 1])
        wr = dict(zip(h["ref_keys"][e0:e1].tolist(), h["ref_w"][e0:e1]))
        d = F32(hl - int(h["ref_bigrams"][ref]))
        pen = np.exp(F32(-(d * d) / F32(72)))
        for n in range(4):
            val = F32(0)
            for k, w in wh[n].items():
                r = wr.get(k, F32(0))
                val = F32(val + F32(min(w, r) * r))
            rn = h["ref_norm"][ref, n]
            if hn[n] != 0 and rn != 0:
                val = F32(val / F32(hn[n] * rn))
            score[n] = F32(score[n] + F32(val * pen))
    s = F32(F32(F32(score[0] + score[1]) + score[2]) + score[3])
    return float(F32(F32(F32(s / F32(4)) / F32(r1 - r0)) * F32(10)))
