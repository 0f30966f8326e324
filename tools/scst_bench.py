"""Self-critical training step of the baseline captioner (capmi.scst) on one MI355X at B = 64 images x n = 5
samples (R = 320 rows), V = 8100, M = H = 512, max_steps = 24 (linear.bias[<end>] - 50, so every row runs all 25
steps and every hypothesis has 25 words: the most work the reward can get), features resident, 5 synthetic
references per image (the decoder's own rollouts under other seeds).

Median of --repeats (>= 20) synchronised runs after a warm-up, host clock around work that ends in a device
synchronise, for each of:

  rollout        BaselineBatchedSampler.sample_device, n samples per image
  reward         capmi_rollout_pack + capmi_cider_reward + capmi_scst_advantage on the rollout's table; the
                 capmi_cider_reward launch alone; and capmi.scst.cider_rewards_host on the same tokens, its
                 device-to-host copy included
  gradient half  pack .. clamp + Adam (everything after the rollouts), issued eagerly and replayed as one graph
  step           the whole step, eager and with graph=True

Every stage runs in a child process of its own under a time limit; the first one that fails ends the run.

python tools/scst_bench.py [--out profiles/scst.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-captioning-with-different-decoders_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

B, N, V, M, H, MAX_STEPS, SEED, REFS = 64, 5, 8100, 512, 512, 24, 5, 5
STAGES = ("rollout", "reward", "gradient_half", "step")
STAGE_TIMEOUT_S = 240


def timed(fn, repeats):
    import torch
    for _ in range(3):  # warm-up: code objects, allocator, lazily made workspaces
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def setup(graph, reward_mix=None):
    """``reward_mix``: the step trains on that mix and the table is a capmi.devscore.ScoreRefs (tools/score_bench.py)."""
    import torch

    import baseline_cases as BLC
    from capmi.optim import Adam
    from capmi.sample import BaselineBatchedSampler
    from capmi.scst import BaselineSelfCriticalStep, CiderRefs
    dev, start, end = "cuda", V - 3, V - 2
    dec, _ = BLC.decoder(M, H, V, SEED, dev, fc_scale=4.0, end_bias=-50.0, end_idx=end)
    dec.fine_tune_embeddings(False)
    feats = torch.rand(B, M, device=dev, generator=torch.Generator(device=dev).manual_seed(SEED)) * 2 - 1
    one = BaselineBatchedSampler(dec, 1)
    refs = [[] for _ in range(B)]
    for seed in range(100, 100 + REFS):
        for b, per in enumerate(one.sample(feats, start, end, max_steps=MAX_STEPS, seed=seed)):
            refs[b].append([w for w in per[0]["seq"] if w not in (start, end, 0)])
    if reward_mix is not None:
        from capmi.devscore import ScoreRefs
        table = ScoreRefs.build(refs, end_idx=end, device=dev)
    else:
        table = CiderRefs.build(refs, end_idx=end, device=dev)
    opt = Adam([q for q in dec.parameters() if q.requires_grad], lr=1e-4)
    opt.set_clip(5.0)

    class Identity(torch.nn.Module):
        def forward(self, x):
            return x

    step = BaselineSelfCriticalStep(Identity(), dec, opt, table, num_samples=N, max_steps=MAX_STEPS, graph=graph,
                                    start_idx=start, end_idx=end, pad_idx=0, reward_mix=reward_mix)
    keys = torch.arange(B, dtype=torch.int32, device=dev)
    return step, feats, keys, table


def run_stage(stage, repeats):
    import torch

    from capmi import kernels as K
    from capmi._lib import CAPMI_SCST_MEAN
    from capmi.scst import cider_rewards_host, hyps_from_table
    if not torch.cuda.is_available():
        raise SystemExit("scst_bench needs the GPU: there is no CPU path to time")
    step, feats, keys, table = setup(False)
    start, end, T, R = V - 3, V - 2, MAX_STEPS + 1, B * N
    row = {}
    if stage == "rollout":
        s = step.sampler
        row["rollout_ms"] = timed(lambda: s.sample_device(feats, start, end, MAX_STEPS, seed=SEED), repeats)
        assert s.last_stats["steps"] == T
        row["rollout_host_syncs"] = s.last_stats["host_syncs"]
    elif stage == "reward":
        step(feats, keys, seed=SEED, update=False)
        sc = step._sc[B]
        ws = sc.ws

        def device_stage():
            K.rollout_pack(sc.tokens, T, R, start, end, 0, sc.lens, sc.caps, ws.count, ws.inv)
            K.cider_reward(sc.tokens, T, R, N, sc.lens, sc.img_key, table, V, end, True, sc.reward)
            K.scst_advantage(sc.reward, None, B, N, CAPMI_SCST_MEAN, sc.adv, sc.stats)

        def host_stage():
            hyps = hyps_from_table(sc.tokens.cpu(), sc.lens.cpu())
            return cider_rewards_host(table, hyps, [r // N for r in range(R)], True, end)

        row["reward_stage_device_ms"] = timed(device_stage, repeats)
        row["cider_reward_launch_ms"] = timed(
            lambda: K.cider_reward(sc.tokens, T, R, N, sc.lens, sc.img_key, table, V, end, True, sc.reward), repeats)
        row["reward_stage_host_ms"] = timed(host_stage, repeats)
        want = torch.tensor(host_stage(), dtype=torch.float64)
        row["reward_max_abs_diff_device_host"] = float((sc.reward.cpu().double() - want).abs().max())
        row["reward_mean"] = float(want.mean())
        row["table_bytes"] = table.nbytes
    elif stage == "gradient_half":
        step(feats, keys, seed=SEED, update=False)
        sc = step._sc[B]
        row["gradient_half_eager_ms"] = timed(lambda: step._grad_half(sc, B, True, True, with_update=True), repeats)
        step.graph_mode = True
        row["gradient_half_replay_ms"] = timed(lambda: step._replay_half(sc, B, (True, True)), repeats)
        assert step.counts["capture"] == 1
    elif stage == "step":
        it = [0]
        rewards = []

        def one(s):
            def f():
                it[0] += 1
                s(feats, keys, seed=SEED + it[0])
                rewards.append(s.last["reward_mean"].clone())
            return f

        row["step_eager_ms"] = timed(one(step), repeats)
        gstep = setup(True)[0]
        row["step_graph_ms"] = timed(one(gstep), repeats)
        assert gstep.counts["capture"] == 1 and gstep.counts["eager"] == 0
        row["reward_mean_over_timed_steps"] = float(torch.cat(rewards).mean())  # for information, not a check
    else:
        raise SystemExit(f"unknown stage {stage}")
    K.sk_check()
    print("STAGE_RESULT " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stage", default=None, choices=STAGES, help="(internal) run one stage in this process")
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if a.stage:
        return run_stage(a.stage, a.repeats)
    res = {"tool": "tools/scst_bench.py", "repeats": a.repeats,
           "shape": {"B": B, "num_samples": N, "V": V, "M": M, "H": H, "max_steps": MAX_STEPS,
                     "references_per_image": REFS}}
    for stage in STAGES:  # a fresh process each, under its own time limit; nothing more is started after a failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", stage, "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=STAGE_TIMEOUT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"stage {stage} failed with exit status {p.returncode}")
        line = [l for l in p.stdout.splitlines() if l.startswith("STAGE_RESULT ")][-1]
        res.update(json.loads(line[len("STAGE_RESULT "):]))
        print(stage, line[len("STAGE_RESULT "):], flush=True)
    res["reward_share_of_step"] = res["reward_stage_device_ms"] / res["step_graph_ms"]
    res["host_reward_over_step"] = res["reward_stage_host_ms"] / res["step_graph_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
