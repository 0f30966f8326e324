"""Captions per second of validation on generated captions (capmi.genval.GeneratedCaptionEval: ``search_device`` +
``DeviceCaptionScorer.score_table`` per batch, one copy of the tables at the end) against the same pass composed from
the host-walk pieces: ``search`` (the state copied to the host and walked in Python per image), then the lists scored
on the same pre-built ``ScoreRefs`` (``DeviceCaptionScorer.corpus_scores``: pack, copy, two launches) or by
``capmi.scoring.caption_scores`` on the host. The reference tables are built once, outside every timed region, and both
device-scored sides read them; the build is timed alone (``refs_build_s``: a pass over new references pays it once on
either side), as is ``caption_scores_device``, which rebuilds the tables on every call. Both captioners, B = 64 images
per batch, k = 3 beams, V = 8100, max_decode_len = 20, seeded weights whose beams never finish (END bias - 50, as
tools/beam_bench.py), so every search runs all 21 steps and every caption is the best live beam's 21 words: the longest
walk and the longest hypotheses the pass can meet at this length. The passes start from the encoder's features: the
encoder forward is the same launches on both sides.
Also timed alone on the state one batch leaves: the back-trace launch (``_BeamState.finish_device``) and the host walk
it replaces (``_BeamState.finish``, its device-to-host copy included).

Each side is warmed up, then the median of --repeats timed runs (host clock around work that ends in a device
synchronise) is taken.

python tools/genval_bench.py [--out profiles/genval.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-captioning-with-different-decoders_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

B, K_BEAM, V, MAX_LEN, SEED, END_BIAS = 64, 3, 8100, 20, 5, -50.0
START, END, PAD = V - 3, V - 2, 0


class Features:
    """The encoder of the timed passes: the batch is its features already."""

    def __call__(self, x):
        return x

    def eval(self):
        return self


def setup(model, n_batches, dev):
    import gen
    from helpers import make_decoder, t
    from capmi.beam import BaselineBatchedBeamSearch, BatchedBeamSearch
    if model == "attention":
        dec, _ = make_decoder(512, 512, 512, V, SEED, dev)
        with torch.no_grad():
            dec.fc.bias[END] += END_BIAS
        feats = [t(gen.encoder_features(SEED + b, B), dev).view(B, 14, 14, 2048) for b in range(n_batches)]
        search, kw = BatchedBeamSearch(dec, K_BEAM), dict(return_alphas=False)
    else:
        import baseline_cases as BLC
        dec, _ = BLC.decoder(512, 512, V, SEED, dev, end_bias=END_BIAS, end_idx=END)
        feats = [t(gen.uniform(SEED + b, "feats", (B, 512), -1, 1), dev) for b in range(n_batches)]
        search, kw = BaselineBatchedBeamSearch(dec, K_BEAM), {}
    dec.eval()
    return dec, feats, search, kw


def timed(fn, repeats):
    fn()  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("genval_bench needs the GPU: there is no CPU path to time")
    if a.repeats < 5:
        raise SystemExit("--repeats must be >= 5")
    from capmi.data import SyntheticCOCO
    from capmi.devscore import DeviceCaptionScorer, ScoreRefs, _cider_listing, caption_scores_device
    from capmi.genval import GeneratedCaptionEval
    from capmi.rollout import AttentionStepper, BaselineStepper
    from capmi.scoring import caption_scores
    from capmi.scst import MAX_REF_WORDS
    dev, N = "cuda", a.batches * B
    ds = SyntheticCOCO(N, V=V, L=25, ragged=True)
    strip = {START, END, PAD}
    references = [[[w for w in cap.tolist() if w not in strip][:MAX_REF_WORDS] for cap in ds.references(i)]
                  for i in range(N)]
    listed = [_cider_listing([tuple(r) for r in rs]) for rs in references]
    refs = ScoreRefs.build(listed, device=dev)
    t_build = timed(lambda: ScoreRefs.build(listed, device=dev), a.repeats)
    scorer = DeviceCaptionScorer(refs)
    rows = []
    for model in ("attention", "baseline"):
        dec, feats, search, kw = setup(model, a.batches, dev)
        last = {}

        def run_device():
            ev = GeneratedCaptionEval(Features(), dec, search, refs, START, END, PAD, max_decode_len=MAX_LEN)
            for b, f in enumerate(feats):
                ev.step(f, range(b * B, (b + 1) * B))
            last["device"] = ev.results()

        def host_captions():
            hyps = []
            for f in feats:
                res = search.search(f, START, END, max_steps=MAX_LEN, **kw)
                for i, r in enumerate(res):
                    seq = r[0] if r[2] else search.last_live[i][0][0]
                    hyps.append([w for w in seq if w not in strip])
            return hyps

        def run_host_scorer():
            last["host"] = caption_scores(references, host_captions())

        def run_host_walk_device_scorer():  # the same tables as the device pass: no build on either side
            last["mixed"] = scorer.corpus_scores(host_captions())

        def run_host_walk_rebuilding_scorer():  # caption_scores_device as it stands: tables rebuilt per call
            last["rebuilt"] = caption_scores_device(references, host_captions(), dev)

        # the state one batch leaves, for the two back-traces alone
        stepper = (AttentionStepper if model == "attention" else BaselineStepper)(dec, feats[0], K_BEAM)
        args = (lambda bs, t_: (bs.live, None)) if model == "attention" else (lambda bs, t_: ())
        state = search._loop(stepper, START, END, MAX_LEN, 8, args)

        t_dev = timed(run_device, a.repeats)
        t_host = timed(run_host_scorer, a.repeats)
        t_mixed = timed(run_host_walk_device_scorer, a.repeats)
        t_rebuilt = timed(run_host_walk_rebuilding_scorer, a.repeats)
        t_bt = timed(lambda: state.finish_device(drop=(START, PAD), fallback_live=True), 20)
        t_walk = timed(lambda: state.finish(False), 20)
        d, h = last["device"], last["host"]
        assert d["hypotheses"] == host_captions()  # the same captions on both sides
        assert all(abs(d[k] - h[k]) <= 1e-9 * abs(h[k]) for k in ("Bleu_1", "Bleu_4", "ROUGE_L"))
        for other in (last["mixed"], last["rebuilt"]):  # same tables, same rows
            assert all(abs(d[k] - v) <= 1e-9 * abs(v) for k, v in other.items())
        md, mh, mm, mr = (statistics.median(x) for x in (t_dev, t_host, t_mixed, t_rebuilt))
        rows.append({"model": model, "images": N, "B": B, "k": K_BEAM, "max_decode_len": MAX_LEN,
                     "repeats": a.repeats, "unfinished": d["unfinished"], "mean_length": d["mean_length"],
                     "device_pass_s": md, "host_walk_host_scorer_s": mh, "host_walk_device_scorer_s": mm,
                     "device_pass_captions_per_s": N / md, "host_walk_host_scorer_captions_per_s": N / mh,
                     "host_walk_device_scorer_captions_per_s": N / mm,
                     "ratio_vs_host_scorer": mh / md, "ratio_vs_device_scorer": mm / md,
                     "host_walk_caption_scores_device_s": mr, "refs_build_s": statistics.median(t_build),
                     "backtrack_launch_ms": 1e3 * statistics.median(t_bt),
                     "finish_host_walk_ms": 1e3 * statistics.median(t_walk),
                     "device_pass_all_s": t_dev, "host_walk_host_scorer_all_s": t_host,
                     "host_walk_device_scorer_all_s": t_mixed, "host_walk_caption_scores_device_all_s": t_rebuilt,
                     "refs_build_all_s": t_build,
                     "scores": {k: d[k] for k in ("Bleu_1", "Bleu_4", "ROUGE_L", "CIDEr")}})
        print(json.dumps(rows[-1]))
    res = {"tool": "tools/genval_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"V": V, "B": B, "k": K_BEAM, "max_decode_len": MAX_LEN, "end_bias": END_BIAS,
                     "attention": {"P": 196, "E": 2048, "A": 512, "D": 512, "M": 512},
                     "baseline": {"M": 512, "H": 512}},
           "results": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
