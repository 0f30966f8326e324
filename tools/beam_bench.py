"""Captions per second of the batched beam search (capmi.beam.BatchedBeamSearch) against a loop of the
single-image BeamSearch.search over the same images, at B in {8, 64}: k = 5, P = 196, E = 2048,
A = D = M = 512, V = 8100, max_steps = 50, seeded weights whose beams never finish (fc.bias[<end>] - 50),
so every search runs all 51 steps. Each side is warmed up, then the median of --repeats timed runs (host
clock around work that ends in a device synchronise) is taken.

python tools/beam_bench.py [--out profiles/beam_batched.json]      both sides, both B, one JSON file
python tools/beam_bench.py --trace-batch 64                         one warmed batched search, for
    rocprofv3 --kernel-trace --stats -- python tools/beam_bench.py --trace-batch 64  (a run of its own)
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

K_BEAM, MAX_STEPS, SEED = 5, 50, 5
A = D = M = 512
V = 8100


def setup(B, dev="cuda"):
    import gen
    from helpers import make_decoder, t
    dec, _ = make_decoder(A, D, M, V, SEED, dev)
    dec.eval()
    start, end = V - 3, V - 2
    with torch.no_grad():
        dec.fc.bias[end] -= 50.0
    feats = t(gen.encoder_features(SEED, B), dev).view(B, 14, 14, 2048)
    return dec, feats, start, end


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
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-batch", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench needs the GPU: there is no CPU path to time")
    from capmi.beam import BatchedBeamSearch, BeamSearch

    if a.trace_batch:
        dec, feats, start, end = setup(a.trace_batch)
        bs = BatchedBeamSearch(dec, K_BEAM)
        for _ in range(2):
            res = bs.search(feats, start, end, max_steps=MAX_STEPS, return_alphas=False)
        torch.cuda.synchronize()
        print(json.dumps({"trace_batch": a.trace_batch, "searches": 2, **bs.last_stats,
                          "finished": sum(r[2] for r in res)}))
        return

    if a.repeats < 5:
        raise SystemExit("--repeats must be >= 5")
    rows = []
    for B in a.batches:
        dec, feats, start, end = setup(B)
        batched, single = BatchedBeamSearch(dec, K_BEAM), BeamSearch(dec, K_BEAM)

        def run_batched():
            return batched.search(feats, start, end, max_steps=MAX_STEPS)

        def run_looped():
            return [single.search(feats[i:i + 1], start, end, max_steps=MAX_STEPS) for i in range(B)]

        fail = ([start, end], [], False)
        assert run_batched() == [fail] * B and run_looped() == [fail] * B  # both run all 51 steps
        assert batched.last_stats["steps"] == MAX_STEPS + 1
        tb, tl = timed(run_batched, a.repeats), timed(run_looped, a.repeats)
        mb, ml = statistics.median(tb), statistics.median(tl)
        rows.append({"B": B, "k": K_BEAM, "steps": MAX_STEPS + 1, "repeats": a.repeats,
                     "batched_s": mb, "looped_s": ml, "batched_captions_per_s": B / mb,
                     "looped_captions_per_s": B / ml, "ratio": ml / mb,
                     "batched_all_s": tb, "looped_all_s": tl, "host_syncs_batched": batched.last_stats["host_syncs"]})
        print(json.dumps(rows[-1]))
    res = {"tool": "tools/beam_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"P": 196, "E": 2048, "A": A, "D": D, "M": M, "V": V, "k": K_BEAM, "max_steps": MAX_STEPS},
           "results": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
