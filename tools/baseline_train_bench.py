"""The baseline captioner's training path, measured (sibling of tools/baseline_eval_bench.py).

step   microseconds per recurrence step at R in {64, 320}, M = H = 512. Forward: capmi_lstm_step_fwd_train (one
       launch) against capmi_gemm TILE_64 + capmi_lstm_cell_fwd. Backward: capmi_lstm_step_bwd (one launch)
       against capmi_lstm_cell_bwd + capmi_gemm TILE_64. One process, the two arms alternating --repeats times;
       each sample is device events around 10 replays of a captured chain of --iters dependent steps (ping-
       ponged state: no host work between launches).
train  milliseconds per decoder training step at B = 64, L = 25, V = 8100 with the image features resident on
       the device (identity encoder): capmi.baseline_train.BaselineTrainStep on a HIP graph against today's loop
       body (BaselineDecoderFn, F.cross_entropy, clamp, torch.optim.Adam, and the sync loss.item() causes), the
       arms alternating in one process; a host clock around --steps synchronised steps. Also images per second
       of the whole step with the ResNet-101 encoder (random weights), graph mode.

python tools/baseline_train_bench.py [--repeats 5] [--out profiles/baseline_train.jsonl]
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

M = H = 512
V, L, B, SEED = 8100, 25, 64, 5


class Identity(torch.nn.Module):
    def forward(self, x):
        return x


def decoder(dev):
    from models.baseline import BaselineDecoder, BaselineDecoderParams
    prm = BaselineDecoderParams()
    prm.embed_size, prm.hidden_size, prm.vocab_size = M, H, V
    torch.manual_seed(SEED)
    dec = BaselineDecoder(prm)
    dec.fine_tune_embeddings(False)  # the default configuration
    return dec.to(dev).train()


def step_times(dec, R, iters, repeats, dev):
    from capmi import kernels as K
    from capmi._lib import CAPMI_A_KMAJOR as AK, CAPMI_B_KROWS as BKR, CAPMI_B_NMAJOR_W as BW
    f = dict(device=dev, dtype=torch.float32)
    g = torch.Generator(device=dev).manual_seed(SEED)
    u = lambda *s: torch.rand(*s, generator=g, **f) * 2 - 1  # noqa: E731
    w_hh = dec.lstm.weight_hh_l0.detach()
    pre, dh = u(R, 4 * H), u(R, H)
    hs, cs = [u(R, H), torch.empty(R, H, **f)], [u(R, H), torch.empty(R, H, **f)]
    act = torch.sigmoid(u(R, 4 * H))
    c_prev, c_cur = u(R, H), u(R, H)
    dgs, dcs = [u(R, 4 * H) * 0.1, torch.empty(R, 4 * H, **f)], [u(R, H), torch.empty(R, H, **f)]
    hh, dhr, act_out = torch.empty(R, 4 * H, **f), torch.empty(R, H, **f), torch.empty(R, 4 * H, **f)

    def fwd(fused, n):
        for i in range(n):
            a, b = i & 1, (i + 1) & 1
            if fused:
                K.lstm_step_fwd_train(R, M, H, hs[b], cs[b], act_out, pre=pre, h_prev=hs[a], c_prev=cs[a], w_hh=w_hh)
            else:
                K.gemm(K.problem(R, 4 * H, H, hs[a], H, w_hh, H, hh, 4 * H), AK, BW, K.TILE_64)
                K.lstm_cell_fwd(pre, 1, 0, None, hh, 1, 0, cs[a], R, H, hs[b], cs[b], act_out)

    def bwd(fused, n):
        for i in range(n):
            a, b = i & 1, (i + 1) & 1
            if fused:
                K.lstm_step_bwd(R, H, act, c_cur, dgs[b], dcs[b], dh_lin=dh, dg_next=dgs[a], w_hh=w_hh, dc_in=dcs[a],
                                c_prev=c_prev)
            else:
                K.gemm(K.problem(R, H, 4 * H, dgs[a], 4 * H, w_hh, H, dhr, H), AK, BKR, K.TILE_64)
                K.lstm_cell_bwd(dh, dhr, 1, 0, dcs[a], act, c_prev, c_cur, R, H, R, dgs[b], dcs[b])

    rows = []
    replays = 10
    for name, run in (("forward_train", fwd), ("backward", bwd)):
        samples = {True: [], False: []}
        graphs = {}
        for fused in (True, False):
            run(fused, 20)
            torch.cuda.synchronize()
            graphs[fused] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[fused]):
                run(fused, iters)
            graphs[fused].replay()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for fused in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _r in range(replays):
                    graphs[fused].replay()
                e1.record()
                torch.cuda.synchronize()
                samples[fused].append(e0.elapsed_time(e1) * 1e3 / (iters * replays))
        row = {"arm": "lstm_train_step", "direction": name, "R": R, "M": M, "H": H, "iters": iters, "replays": replays,
               "repeats": repeats, "timing": "device events around graph replays"}
        for fused, key in ((True, "fused_us"), (False, "sequence_us")):
            s = samples[fused]
            row[key] = statistics.median(s)
            row[key + "_min_max"] = [min(s), max(s)]
        row["sequence_over_fused"] = row["sequence_us"] / row["fused_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def train_times(steps, repeats, dev, with_encoder):
    from capmi.baseline_train import BaselineTrainStep
    from capmi.optim import Adam
    g = torch.Generator(device=dev).manual_seed(SEED)
    feats = torch.rand(B, M, generator=g, device=dev) * 2 - 1
    caps = torch.randint(1, V, (B, L), generator=g, device=dev)
    caps[B // 2:, L - 5:] = 0  # PAD tails
    dec1, dec2 = decoder(dev), decoder(dev)
    opt1 = Adam([q for q in dec1.parameters() if q.requires_grad], lr=1e-4)
    opt1.set_clip(5.0)
    step = BaselineTrainStep(Identity(), dec1, opt1, graph=True)
    opt2 = torch.optim.Adam([q for q in dec2.parameters() if q.requires_grad], lr=1e-4)

    def arm_step(n):
        for _ in range(n):
            step(feats, caps)

    def arm_loop(n):
        for _ in range(n):
            scores = dec2(feats, caps)
            loss = torch.nn.functional.cross_entropy(scores.reshape(-1, V), caps.reshape(-1), ignore_index=0)
            opt2.zero_grad()
            loss.backward()
            for q in opt2.param_groups[0]["params"]:
                q.grad.data.clamp_(-5.0, 5.0)
            opt2.step()
            loss.item()

    arms = {"BaselineTrainStep_graph": arm_step, "autograd_loop": arm_loop}
    times = {k: [] for k in arms}
    for fn in arms.values():
        fn(3)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    rows = []
    for k, ts in times.items():
        rows.append({"arm": k, "B": B, "L": L, "V": V, "M": M, "H": H, "steps": steps, "repeats": repeats,
                     "ms_per_step": statistics.median(ts), "min_max": [min(ts), max(ts)],
                     "timing": "host clock around synchronised steps, features resident"})
    rows[0]["loop_over_step"] = rows[1]["ms_per_step"] / rows[0]["ms_per_step"]
    rows[0]["counts"] = dict(step.counts)
    for r in rows:
        print(json.dumps(r), flush=True)
    if with_encoder:
        from models.encoder import Encoder
        torch.manual_seed(SEED)
        enc = Encoder(M).to(dev).train()
        dec3 = decoder(dev)
        opt3 = Adam([q for q in dec3.parameters() if q.requires_grad], lr=1e-4)
        opt3.set_clip(5.0)
        full = BaselineTrainStep(enc, dec3, opt3, graph=True)
        imgs = torch.rand(B, 3, 224, 224, generator=g, device=dev)
        full(imgs, caps)
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _s in range(5):
                full(imgs, caps)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / 5)
        row = {"arm": "whole_step_with_encoder_graph", "B": B, "ms_per_step": statistics.median(ts) * 1e3,
               "images_per_s": B / statistics.median(ts), "timing": "host clock around synchronised steps"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["step", "train", "both"], default="both")
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 320])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no_encoder", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("baseline_train_bench needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    rows = []
    if a.what in ("step", "both"):
        dec = decoder(dev)
        for R in a.rows:
            rows += step_times(dec, R, a.iters, a.repeats, dev)
    if a.what in ("train", "both"):
        rows += train_times(a.steps, a.repeats, dev, not a.no_encoder)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps({"tool": "tools/baseline_train_bench.py", "device": torch.cuda.get_device_name(0),
                                "shape": {"M": M, "H": H, "V": V, "B": B, "L": L}, "results": rows}) + "\n")


if __name__ == "__main__":
    main()
