"""Sampled rollouts (capmi.sample) at B = 64 images x num_samples = 5 (R = 320 rows), V = 8100, 25 steps
(max_steps = 24; fc.bias[<end>] - 50, so every row runs all of them): the capmi_sample_step launch against the
same sampling stage composed from torch ops (log_softmax, topk, multinomial, gather, masked updates) inside the
same rollout, in the same process, for the attention decoder (P = 196, E = 2048, A = D = M = 512) and the
baseline decoder (M = H = 512).

Per setting (temperature, top_k): us of the capmi_sample_step dispatch alone (its own start / end timestamps), us
per sampling stage as the loop issues it (device events around --launches back-to-back stages on fixed logits,
so the host's launch cost is in it on both sides), ms per full rollout and captions / s (host clock around a
rollout that ends in a device synchronise). Each side is warmed up; the figures are medians of --repeats (>= 20) timed runs.

python tools/sample_bench.py [--out profiles/sample.json]
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

B, N, V, MAX_STEPS, SEED = 64, 5, 8100, 24, 5
A = D = M = 512
SETTINGS = ((1.0, 0), (0.8, 10))


class TorchStage:
    """The sampling stage from torch ops, in place of the capmi_sample_step launch (mixed in before a sampler):
    the same outputs into the same tables, the draw by torch.multinomial."""

    def _draw(self, logits, t_, V_, end_idx, prev):
        lp = torch.log_softmax(logits / self.temperature, 1)
        if 0 < self.top_k < V_:
            v, idx = lp.topk(self.top_k, 1)
            v = torch.log_softmax(v, 1)
            choice = torch.multinomial(v.exp(), 1)
            tok, tlp = idx.gather(1, choice).view(-1), v.gather(1, choice).view(-1)
        else:
            tok = torch.multinomial(lp.exp(), 1)
            tlp, tok = lp.gather(1, tok).view(-1), tok.view(-1)
        alive = self.alive.bool()
        self.tokens[t_] = torch.where(alive, tok.int(), self.tokens[t_])
        self.logp[t_] = torch.where(alive, tlp, self.logp[t_])
        prev.copy_(torch.where(alive, tok, prev))
        ended = alive & (tok == end_idx)
        self.alive.sub_(ended.int())
        self.rows_live.sub_(ended.sum().int())
        self.steps += 1
        if self.steps % self.sync_every == 0 and self.steps < self.T:
            self.syncs += 1
            return int(self.rows_live.item()) == 0
        return False


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


def stage_us(sampler, logits, launches, repeats):
    """median us per sampling stage: ``launches`` stages back to back between two device events"""
    R = logits.size(0)
    sampler._begin(logits.device, R // sampler.n, V, 0, 1, None, False, 1 << 30)
    prev = torch.zeros(R, dtype=torch.int64, device=logits.device)

    def burst():
        for _ in range(launches):
            sampler._draw(logits, 0, V, -1, prev)

    burst()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        burst()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return statistics.median(out)


def kernel_us(sampler, logits, repeats):
    """median us of the capmi_sample_step dispatch itself (the packet's own start / end timestamps)"""
    from capmi import kernels as K
    R = logits.size(0)
    sampler._begin(logits.device, R // sampler.n, V, 0, 1, None, False, 1 << 30)
    prev = torch.zeros(R, dtype=torch.int64, device=logits.device)
    out = []
    for i in range(repeats + 3):
        e0, e1 = K.TimingEvent(), K.TimingEvent()
        K.timed_launch(lambda: sampler._draw(logits, 0, V, -1, prev), e0, e1)
        torch.cuda.synchronize()
        if i >= 3:
            out.append(e0.elapsed_ms(e1) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs the GPU: there is no CPU path to time")
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    import baseline_cases as BLC
    import gen
    from helpers import make_decoder, t
    from capmi.sample import BaselineBatchedSampler, BatchedSampler

    class TorchBatchedSampler(TorchStage, BatchedSampler):
        pass

    class TorchBaselineBatchedSampler(TorchStage, BaselineBatchedSampler):
        pass

    dev, start, end = "cuda", V - 3, V - 2
    dec, _ = make_decoder(A, D, M, V, SEED, dev)
    dec.eval()
    bdec, _ = BLC.decoder(M, D, V, SEED, dev, end_bias=-50.0, end_idx=end)
    with torch.no_grad():
        dec.fc.bias[end] -= 50.0
    feats = t(gen.encoder_features(SEED, B), dev).view(B, 14, 14, 2048)
    bfeats = torch.rand(B, M, device=dev, generator=torch.Generator(device=dev).manual_seed(SEED)) * 2 - 1
    logits = 3.0 * torch.randn(B * N, V, device=dev, generator=torch.Generator(device=dev).manual_seed(SEED))
    rows = []
    for temperature, top_k in SETTINGS:
        row = {"temperature": temperature, "top_k": top_k, "B": B, "num_samples": N, "steps": MAX_STEPS + 1,
               "repeats": a.repeats}
        row["sample_step_kernel_us"] = kernel_us(BaselineBatchedSampler(bdec, N, temperature, top_k), logits,
                                                 a.repeats)
        row["sample_step_us"] = stage_us(BaselineBatchedSampler(bdec, N, temperature, top_k), logits, a.launches,
                                         a.repeats)
        row["torch_stage_us"] = stage_us(TorchBaselineBatchedSampler(bdec, N, temperature, top_k), logits,
                                         a.launches, a.repeats)
        for name, kern, comp, x in (("attention", BatchedSampler(dec, N, temperature, top_k),
                                     TorchBatchedSampler(dec, N, temperature, top_k), feats),
                                    ("baseline", BaselineBatchedSampler(bdec, N, temperature, top_k),
                                     TorchBaselineBatchedSampler(bdec, N, temperature, top_k), bfeats)):
            for side, s in (("kernel", kern), ("torch", comp)):
                out = s.sample(x, start, end, max_steps=MAX_STEPS, seed=SEED)
                assert s.last_stats["steps"] == MAX_STEPS + 1  # every row runs all 25 steps on both sides
                assert all(len(d["seq"]) == MAX_STEPS + 1 and not d["finished"] for per in out for d in per)
                ts = timed(lambda s=s, x=x: s.sample(x, start, end, max_steps=MAX_STEPS, seed=SEED), a.repeats)
                ms = statistics.median(ts) * 1e3
                row[f"{name}_{side}_rollout_ms"] = ms
                row[f"{name}_{side}_captions_per_s"] = B * N / (ms * 1e-3)
                row[f"{name}_{side}_host_syncs"] = s.last_stats["host_syncs"]
            row[f"{name}_ratio"] = row[f"{name}_torch_rollout_ms"] / row[f"{name}_kernel_rollout_ms"]
        rows.append(row)
        print(json.dumps(row))
    res = {"tool": "tools/sample_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "num_samples": N, "V": V, "max_steps": MAX_STEPS, "P": 196, "E": 2048, "A": A, "D": D,
                     "M": M, "baseline_H": D}, "results": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
