"""The caption metrics on the device (capmi.devscore, csrc/score.hip) on one MI355X, by the method of
tools/scst_bench.py: median of --repeats (>= 20) synchronised runs after a warm-up, host clock around work that ends
in a device synchronise (the host scorer, which takes seconds, is run --host_repeats times).

  scorer   capmi.scoring.caption_scores against capmi.devscore.caption_scores_device on the same lists in the same
           run: 5000 synthetic images (V = 8100, references of 8..16 words, the hypothesis a noisy copy of one of
           them), once with 5 distinct references per image and once with one reference listed 20 times (what the
           validation pass builds). The device scorer with its table build (what validation pays) and on tables
           already built; the largest difference of the six scores between the two scorers.
  launch   capmi_caption_stats alone at R = 320, T = 25, 5 references per image (the table of tools/scst_bench.py's
           step), next to capmi_cider_reward and capmi_reward_mix on the same table.
  step     the self-critical step of the baseline captioner (tools/scst_bench.py's shape) as one graph, trained on
           CIDEr-D alone and on a mix of the three metrics; the gradient half alone likewise.

Every stage runs in a child process of its own under a time limit; the first one that fails ends the run.

python tools/score_bench.py [--out profiles/score.json]
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scst_bench as SB  # noqa: E402  (also puts the package and the tests' helpers on sys.path)

IMAGES, V = 5000, 8100
STAGES = ("scorer", "launch", "step")
STAGE_TIMEOUT_S = 400
MIX = dict(cider=1.0, bleu4=0.5, rouge_l=0.25)
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")


def corpus(kind):
    """(references, hypotheses) of IMAGES images: ``distinct5`` or ``repeated20``"""
    rng = random.Random(11)
    references, hypotheses = [], []
    for _ in range(IMAGES):
        caps = [[rng.randint(3, V - 1) for _ in range(rng.randint(8, 16))] for _ in range(5)]
        for c in caps[1:]:  # references of one image share words
            for j in range(min(len(c), len(caps[0]))):
                if rng.random() < 0.5:
                    c[j] = caps[0][j]
        hypotheses.append([w if rng.random() < 0.7 else rng.randint(3, V - 1) for w in caps[0] if rng.random() < 0.9])
        references.append(caps if kind == "distinct5" else [caps[0]] * 20)
    return references, hypotheses


def host_timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def run_stage(stage, repeats, host_repeats):
    import torch

    from capmi import kernels as K
    from capmi.devscore import DeviceCaptionScorer, ScoreRefs, _cider_listing, caption_scores_device
    from capmi.scoring import caption_scores
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs the GPU")
    row = {}
    if stage == "scorer":
        for kind in ("distinct5", "repeated20"):
            references, hypotheses = corpus(kind)
            host = caption_scores(references, hypotheses)
            dev = caption_scores_device(references, hypotheses, "cuda")
            listed = [_cider_listing([tuple(r) for r in refs]) for refs in references]
            scorer = DeviceCaptionScorer(ScoreRefs.build(listed, device="cuda"))
            row[kind] = dict(
                host_ms=host_timed(lambda: caption_scores(references, hypotheses), host_repeats),
                device_with_table_build_ms=SB.timed(lambda: caption_scores_device(references, hypotheses, "cuda"),
                                                    repeats),
                table_build_ms=SB.timed(lambda: ScoreRefs.build(listed, device="cuda"), repeats),
                device_tables_built_ms=SB.timed(lambda: scorer.corpus_scores(hypotheses), repeats),
                table_bytes=scorer.refs.nbytes,
                max_rel_diff_device_host=max(abs(dev[k] - host[k]) / abs(host[k]) for k in KEYS),
                scores_host=host)
    elif stage == "launch":
        step, feats, keys, table = SB.setup(False, MIX)
        step(feats, keys, seed=SB.SEED, update=False)
        sc = step._sc[SB.B]
        T, R, end = SB.MAX_STEPS + 1, SB.B * SB.N, V - 2
        row["caption_stats_launch_ms"] = SB.timed(
            lambda: K.caption_stats(sc.tokens, T, R, SB.N, sc.lens, sc.img_key, table, V, end, True, sc.score_stats,
                                    sc.bleu, sc.rouge), repeats)
        row["cider_reward_launch_ms"] = SB.timed(
            lambda: K.cider_reward(sc.tokens, T, R, SB.N, sc.lens, sc.img_key, table.cider, V, end, True, sc.cider),
            repeats)
        row["reward_mix_launch_ms"] = SB.timed(
            lambda: K.reward_mix(sc.cider, sc.bleu, sc.rouge, R, 1.0, 0.5, 0.25, sc.reward), repeats)
        row["empty_sync_ms"] = SB.timed(lambda: None, repeats)  # what the clock and the synchronise cost alone
        row["launch_shape"] = dict(R=R, T=T, references_per_image=SB.REFS, hypothesis_words=int(sc.lens.max()))
        row["launch_table_bytes"] = table.nbytes
    elif stage == "step":
        for name, mix in (("cider", None), ("mix", MIX)):
            it = [0]
            gstep, feats, keys, _ = SB.setup(True, mix)

            def one():
                it[0] += 1
                gstep(feats, keys, seed=SB.SEED + it[0])

            row[f"step_graph_{name}_ms"] = SB.timed(one, repeats)
            assert gstep.counts["capture"] == 1 and gstep.counts["eager"] == 0
            sc = gstep._sc[SB.B]
            row[f"gradient_half_replay_{name}_ms"] = SB.timed(lambda: gstep._replay_half(sc, SB.B, (True, True)),
                                                              repeats)
    else:
        raise SystemExit(f"unknown stage {stage}")
    K.sk_check()
    print("STAGE_RESULT " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host_repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stage", default=None, choices=STAGES, help="(internal) run one stage in this process")
    a = ap.parse_args()
    if a.repeats < 20 or a.host_repeats < 3:
        raise SystemExit("--repeats must be >= 20 and --host_repeats >= 3")
    if a.stage:
        return run_stage(a.stage, a.repeats, a.host_repeats)
    res = {"tool": "tools/score_bench.py", "repeats": a.repeats, "host_repeats": a.host_repeats,
           "scorer_shape": {"images": IMAGES, "V": V, "reference_words": "8..16"}, "reward_mix": MIX}
    for stage in STAGES:  # a fresh process each, under its own time limit; nothing more is started after a failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", stage, "--repeats", str(a.repeats),
                            "--host_repeats", str(a.host_repeats)], capture_output=True, text=True,
                           timeout=STAGE_TIMEOUT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"stage {stage} failed with exit status {p.returncode}")
        line = [l for l in p.stdout.splitlines() if l.startswith("STAGE_RESULT ")][-1]
        res.update(json.loads(line[len("STAGE_RESULT "):]))
        print(stage, line[len("STAGE_RESULT "):], flush=True)
    for kind in ("distinct5", "repeated20"):
        res[kind]["host_over_device_with_build"] = res[kind]["host_ms"] / res[kind]["device_with_table_build_ms"]
    res["stats_launch_over_cider_launch"] = res["caption_stats_launch_ms"] / res["cider_reward_launch_ms"]
    res["mix_step_over_cider_step"] = res["step_graph_mix_ms"] / res["step_graph_cider_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
