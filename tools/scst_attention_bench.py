"""Self-critical training step of the attention captioner (capmi.scst.AttentionSelfCriticalStep) on one MI355X at
B = 64 images x n = 5 samples (R = 320 rows), V = 8100, A = D = M = 512, E = 2048, P = 196 and P = 49 feature
positions, max_steps = 24 (fc.bias[<end>] - 50, so every row runs all 25 steps), features resident, 5 synthetic
references per image (the decoder's own rollouts under other seeds), the teacher-forced GEMMs in bench.py's
'fp32-x3' arithmetic (the rollouts' GEMMs are fp32 MFMA).

Median of --repeats (>= 20) synchronised runs after a warm-up, host clock around work that ends in a device
synchronise, for each P and each of:

  rollout        BatchedSampler.sample_device, n samples per image
  reward         capmi_rollout_pack + capmi_cider_reward + capmi_scst_advantage on the rollout's table
  gradient half  pack .. clamp + Adam on capmi.decoder_group (features once per image), issued eagerly and
                 replayed as one graph; peak device memory of the process
  replicated     the comparison arm, built here and not in the library: the same gradient half on the existing
                 DecoderCore with the features repeat_interleave'd n times (the copy is part of the arm), eager
                 and replayed; peak device memory of the process
  kernels        capmi_att_group_bwd and capmi_att_group_enc_grad alone, per call inside a replayed graph of T
                 calls; beside them the kernels the replicated arm runs in their place (att_ctx_bwd +
                 att_score_bwd, att_enc_grad on R rows of replicated features)
  step           the whole step, eager and with graph=True

``bytes`` holds the feature traffic computed from the shapes (not measured): what one pass over enc / att_enc
costs once per image and once per row, and the per-step reads of the backward kernels.

Every stage runs in a child process of its own under a time limit; the first one that fails ends the run.

python tools/scst_attention_bench.py [--out profiles/scst_attention.json]
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

B, N, V, A, D, M, E, MAX_STEPS, SEED, REFS = 64, 5, 8100, 512, 512, 512, 2048, 24, 5, 5
PS = (196, 49)
PRECISION = "fp32-x3"
STAGES = ("rollout", "reward", "gradient_half", "replicated", "kernels", "step")
STAGE_TIMEOUT_S = 300


def shape_bytes(P):
    """Feature bytes from the shapes: enc and att_enc once per image and once per row, and what T steps of
    forward (context, scores) plus backward (att_ctx_bwd reads enc, att_score_bwd reads att_enc) read of them."""
    T, R = MAX_STEPS + 1, B * N
    enc, att = B * P * E * 4, B * P * A * 4
    return dict(enc_once=enc, att_enc_once=att, enc_per_row=enc * N, att_enc_per_row=att * N,
                feature_reads_all_steps_once=2 * T * (enc + att), feature_reads_all_steps_per_row=2 * T * N * (enc + att),
                T=T, R=R)


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


def graphed(fn):
    """``fn`` captured once (after a warm pass on a side stream); returns the replay."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def setup(P, graph):
    import torch

    from capmi.optim import Adam
    from capmi.sample import BatchedSampler
    from capmi.scst import AttentionSelfCriticalStep, CiderRefs
    from helpers import make_decoder
    dev, start, end = "cuda", V - 3, V - 2
    dec, _ = make_decoder(A, D, M, V, SEED, dev)
    with torch.no_grad():
        dec.fc.weight.mul_(4.0)
        dec.fc.bias[end] -= 50.0
    dec.fine_tune_embeddings(False)
    dec.set_compute_precision(PRECISION)  # bench.py's decoder arithmetic; both arms follow it
    dec.train()
    feats = torch.rand(B, P, E, device=dev, generator=torch.Generator(device=dev).manual_seed(SEED))
    one = BatchedSampler(dec, 1)
    refs = [[] for _ in range(B)]
    for seed in range(100, 100 + REFS):
        for b, per in enumerate(one.sample(feats, start, end, max_steps=MAX_STEPS, seed=seed)):
            refs[b].append([w for w in per[0]["seq"] if w not in (start, end, 0)])
    table = CiderRefs.build(refs, end_idx=end, device=dev)
    opt = Adam([q for q in dec.parameters() if q.requires_grad], lr=1e-4)
    opt.set_clip(5.0)

    class Feats(torch.nn.Module):
        def forward(self, x):
            return x

    step = AttentionSelfCriticalStep(Feats(), dec, opt, table, num_samples=N, max_steps=MAX_STEPS, graph=graph,
                                     start_idx=start, end_idx=end, pad_idx=0)
    keys = torch.arange(B, dtype=torch.int32, device=dev)
    return step, feats, keys, table


def replicated_half(step, sc):
    """The gradient half of ``step`` with DecoderCore on features repeated n times in place of capmi.decoder_group."""
    from capmi import decoder_fn as DF
    from capmi import kernels as K
    from capmi._lib import CAPMI_SCST_MEAN
    T, R, end = MAX_STEPS + 1, B * N, V - 2
    ws, dec = sc.ws, step.decoder
    p = DF.decoder_params(dec)
    named = dict(dec.named_parameters())
    grads = {k: named[k].grad for k in step.need}
    grads["attention.full_att.weight"] = grads["attention.full_att.weight"].view(-1)

    def half():
        K.rollout_pack(sc.tokens, T, R, V - 3, end, 0, sc.lens, sc.caps, ws.count, ws.inv)
        K.cider_reward(sc.tokens, T, R, N, sc.lens, sc.img_key, step.refs, V, end, True, sc.reward)
        K.scst_advantage(sc.reward, None, B, N, CAPMI_SCST_MEAN, sc.adv, sc.stats)
        enc = sc.feats.repeat_interleave(N, 0)
        preds, _, st = DF.CORE.forward(p, enc, sc.caps, [T] * R, gemm_flags=DF.gemm_flags(dec))
        K.pg_ce_fwd_bwd(preds, sc.caps, R, T, T + 1, V, 1, sc.lens, 0, sc.adv, ws.inv, sc.logp_rows, ws.loss_rows,
                        ws.dlogits, True)
        K.loss_finalize_dev(ws.loss_rows, R * T, ws.inv, ws.loss)
        DF.CORE.backward(p, st, grads, ws.dlogits, dpred_time_major=True, need=step.need)
        step.opt.step()
    return half


def run_stage(stage, P, repeats):
    import torch

    from capmi import kernels as K
    from capmi._lib import CAPMI_SCST_MEAN
    if not torch.cuda.is_available():
        raise SystemExit("scst_attention_bench needs the GPU: there is no CPU path to time")
    step, feats, keys, table = setup(P, False)
    start, end, T, R = V - 3, V - 2, MAX_STEPS + 1, B * N
    row = {}
    if stage == "rollout":
        s = step.sampler
        row["rollout_ms"] = timed(lambda: s.sample_device(feats, start, end, MAX_STEPS, seed=SEED), repeats)
        assert s.last_stats["steps"] == T
    elif stage == "reward":
        step(feats, keys, seed=SEED, update=False)
        sc = step._sc[B]

        def device_stage():
            K.rollout_pack(sc.tokens, T, R, start, end, 0, sc.lens, sc.caps, sc.ws.count, sc.ws.inv)
            K.cider_reward(sc.tokens, T, R, N, sc.lens, sc.img_key, table, V, end, True, sc.reward)
            K.scst_advantage(sc.reward, None, B, N, CAPMI_SCST_MEAN, sc.adv, sc.stats)

        row["reward_stage_device_ms"] = timed(device_stage, repeats)
        row["reward_mean"] = float(sc.reward.mean())
    elif stage == "gradient_half":
        torch.cuda.reset_peak_memory_stats()
        step(feats, keys, seed=SEED, update=False)
        sc = step._sc[B]
        row["gradient_half_eager_ms"] = timed(lambda: step._grad_half(sc, B, True, True, with_update=True), repeats)
        step.graph_mode = True
        row["gradient_half_replay_ms"] = timed(lambda: step._replay_half(sc, B, (True, True)), repeats)
        assert step.counts["capture"] == 1
        row["gradient_half_peak_mb"] = torch.cuda.max_memory_allocated() / 2 ** 20
        row["loss"] = float(sc.ws.loss)
    elif stage == "replicated":
        torch.cuda.reset_peak_memory_stats()
        # the rollout and the buffers of the step, without its grouped pass
        with torch.no_grad():
            sc = step._sc_buffers(B, feats)
            sc.feats.copy_(feats)
            sc.img_key.copy_(keys)
            sc.tokens.copy_(step.sampler.sample_device(sc.feats, start, end, MAX_STEPS, seed=SEED)[0])
        half = replicated_half(step, sc)
        row["replicated_half_eager_ms"] = timed(half, repeats)
        row["replicated_half_replay_ms"] = timed(graphed(half), repeats)
        row["replicated_half_peak_mb"] = torch.cuda.max_memory_allocated() / 2 ** 20
        row["replicated_loss"] = float(sc.ws.loss)
    elif stage == "kernels":
        step(feats, keys, seed=SEED, update=False)
        sc = step._sc[B]
        ws = next(iter(sc.core._ws.values()))
        wf = step.decoder.attention.full_att.weight.view(-1)
        s_dx = ws.P_dx.shape[0]

        def group_bwd():
            for t in range(T):
                K.att_group_bwd(ws.P_dx, s_dx, R * E, ws.GATE[t], ws.AWE[t], sc.feats, ws.ALPHA[t], P, ws.ATT_ENC,
                                ws.AD[t], wf, B, N, P, A, E, ws.DALPHA, ws.DGP[t], ws.DE[t], ws.DAD[t])

        def group_enc_grad():
            K.att_group_enc_grad(ws.DE, ws.ATT_ENC, ws.AD, wf, T, B, N, P, A, ws.DATT, ws.WF_PART, ws.BF_PART)

        row["att_group_bwd_ms"] = timed(graphed(group_bwd), repeats) / T
        row["att_group_enc_grad_ms"] = timed(graphed(group_enc_grad), repeats)
        # what the replicated arm runs in their place, on n-fold copies
        enc_r, att_r = sc.feats.repeat_interleave(N, 0), ws.ATT_ENC.repeat_interleave(N, 0)
        datt = torch.empty(R, P, A, device="cuda")
        nblk = K.att_enc_grad_blocks(R, P)
        wfp, bfp = torch.empty(nblk, A, device="cuda"), torch.empty(nblk, 1, device="cuda")

        def rows_bwd():
            for t in range(T):
                K.att_ctx_bwd(ws.P_dx, s_dx, R * E, ws.GATE[t], ws.AWE[t], enc_r, R, P, E, ws.DGP[t], ws.DALPHA)
                K.att_score_bwd(ws.DALPHA, None, 0, ws.ALPHA[t], P, att_r, ws.AD[t], wf, R, P, A, R, ws.DE[t], ws.DAD[t])

        def rows_enc_grad():
            K.att_enc_grad(ws.DE, att_r, ws.AD, wf, T, R, P, A, datt, wfp, bfp)

        row["att_ctx_score_bwd_rows_ms"] = timed(graphed(rows_bwd), repeats) / T
        row["att_enc_grad_rows_ms"] = timed(graphed(rows_enc_grad), repeats)
    elif stage == "step":
        it = [0]

        def one(s):
            def f():
                it[0] += 1
                s(feats, keys, seed=SEED + it[0])
            return f

        row["step_eager_ms"] = timed(one(step), repeats)
        gstep = setup(P, True)[0]
        row["step_graph_ms"] = timed(one(gstep), repeats)
        assert gstep.counts["capture"] == 1 and gstep.counts["eager"] == 0
    else:
        raise SystemExit(f"unknown stage {stage}")
    K.sk_check()
    print("STAGE_RESULT " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stage", default=None, choices=STAGES, help="(internal) run one stage in this process")
    ap.add_argument("--P", type=int, default=PS[0], help="(internal) feature positions of the stage")
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if a.stage:
        return run_stage(a.stage, a.P, a.repeats)
    res = {"tool": "tools/scst_attention_bench.py", "repeats": a.repeats,
           "shape": {"B": B, "num_samples": N, "V": V, "A": A, "D": D, "M": M, "E": E, "max_steps": MAX_STEPS,
                     "references_per_image": REFS, "decoder_gemm_arithmetic": PRECISION}}
    for P in PS:
        r = res[f"P{P}"] = {"bytes": shape_bytes(P)}
        for stage in STAGES:  # a fresh process each, under its own time limit; nothing more is started after a failure
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", stage, "--P", str(P), "--repeats",
                                str(a.repeats)], capture_output=True, text=True, timeout=STAGE_TIMEOUT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"stage {stage} (P = {P}) failed with exit status {p.returncode}")
            line = [l for l in p.stdout.splitlines() if l.startswith("STAGE_RESULT ")][-1]
            r.update(json.loads(line[len("STAGE_RESULT "):]))
            print(P, stage, line[len("STAGE_RESULT "):], flush=True)
        r["grouped_over_replicated_replay"] = r["gradient_half_replay_ms"] / r["replicated_half_replay_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
