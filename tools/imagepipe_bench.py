"""What the device image cache (capmi.imagepipe.DeviceImageCache, train.py --image_cache_gb) buys:
the host's JPEG decode rate, the per-batch image work with and without the cache, and the attention train()
over a small COCO-shaped tree with the cache off and on. The tree (640x480 quality-92 JPEGs, five 10-word
captions per image, a vocabulary over their words) is written to a temporary directory with PIL.

  (a) decode only     images/s of a DataLoader whose workers do nothing but capmi.imagepipe.decode_rgb, at 1 and
                      --workers workers (host clock over --decode-passes passes of the tree, after one warm-up pass)
  (b) batch of 64     ms per call, all arms warmed up, then run in turn --repeats times (host clock around --calls
                      calls ending in a device synchronise; medians and every repeat are reported):
                        GpuImageTransform   the uncached path on 64 decoded 640x480 images (pinned source: upload of
                                            the 59 MB of pixels, two resample passes, normalise)
                        cache, all hit      DeviceImageCache.__call__ with no pixels: table lookup, index upload, gather
                        gather kernel       the bare capmi_gather_normalize_u8 launch on a resident index tensor; also
                                            device events around a HIP graph of 10 * --calls such launches (no host
                                            between them): TB/s = (64 * 150,528 B read + 64 * 602,112 B written =
                                            48.2 MB) over that time per launch
  (c) train()         models.attention.train, two epochs of --train-images images x 5 captions, batch 64, with
                      --image_cache_gb 0 and 1, each in a process of its own: seconds, images/s and JPEG decodes of each
                      epoch (decodes are counted in the loader workers, epochs end where train() saves its checkpoint;
                      epoch 1 includes the graph captures), and the rate after the epoch's first batch, which leaves
                      out the start of that epoch's loader workers

python tools/imagepipe_bench.py [--workers 16] [--train-workers 12] [--train-images 512] [--out profiles/image_cache.json]
"""
import argparse
import json
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-captioning-with-different-decoders_amd"))

WORDS = ("a man dog cat bird bus street plate food bench wave board red two people on of the near with big small "
         "riding sitting standing holding table field water grass").split()


def write_tree(root, n_img, seed=0):
    """images/NNNNNN.jpg + captions.json + vocab.pkl; every caption has 10 words (one batch shape per batch size)."""
    from PIL import Image
    from vocabulary import END_TOKEN, PAD_TOKEN, START_TOKEN, UNK_TOKEN, Vocabulary
    rng = np.random.default_rng(seed)
    img_dir = os.path.join(root, "images")
    os.makedirs(img_dir)
    images, anns = [], []
    for i in range(n_img):
        # smooth colour fields plus noise: about 155 KB at quality 92, the size of a COCO photograph (white noise: 300 KB)
        low = Image.fromarray(rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)).resize((640, 480), Image.BICUBIC)
        a = np.clip(np.asarray(low).astype(np.int16) + rng.integers(-25, 26, (480, 640, 3)), 0, 255).astype(np.uint8)
        name = f"{i:06d}.jpg"
        Image.fromarray(a).save(os.path.join(img_dir, name), quality=92)
        images.append({"id": 1000 + i, "file_name": name, "height": 480, "width": 640})
        for j in range(5):
            cap = " ".join(rng.choice(WORDS, 10))
            anns.append({"id": 5 * i + j, "image_id": 1000 + i, "caption": cap})
    anno = os.path.join(root, "captions.json")
    with open(anno, "w") as f:
        json.dump({"images": images, "annotations": anns}, f)
    vocab = Vocabulary()
    vocab.add_word(PAD_TOKEN)
    for w in WORDS:
        vocab.add_word(w)
    for t in (START_TOKEN, END_TOKEN, UNK_TOKEN):
        vocab.add_word(t)
    vf = os.path.join(root, "vocab.pkl")
    with open(vf, "wb") as f:
        pickle.dump(vocab, f)
    return anno, img_dir, vf, vocab


class DecodeOnly(torch.utils.data.Dataset):
    def __init__(self, paths):
        self.paths = paths

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from capmi.imagepipe import decode_rgb
        return decode_rgb(self.paths[i]).shape[0]


def decode_rate(paths, workers, passes):
    loader = torch.utils.data.DataLoader(DecodeOnly(paths), batch_size=64, num_workers=workers,
                                         persistent_workers=True, collate_fn=len)
    n = sum(loader)  # warm-up pass: workers started, files in the page cache
    t0 = time.perf_counter()
    for _ in range(passes):
        n = sum(loader)
    dt = time.perf_counter() - t0
    del loader
    return passes * n / dt


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def graph_of(fn, calls):
    """`calls` launches of fn captured into one HIP graph: replayed, they run back to back with no host in between."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def event_timed(graph, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def summary(xs):
    return {"median": round(statistics.median(xs), 5), "min": round(min(xs), 5), "max": round(max(xs), 5),
            "repeats": [round(x, 5) for x in xs]}


def batch_arms(paths, dev, args):
    from capmi import kernels as K
    from capmi.imagepipe import MEAN, STD, DeviceImageCache, GpuImageTransform, PackedImages, decode_rgb
    B = 64
    arrs = [decode_rgb(p) for p in paths[:B]]
    packed = PackedImages(arrs)  # pinned
    tf = GpuImageTransform(dev)
    cache = DeviceImageCache(dev, 2 * B, B)
    keys = list(range(B))
    want = tf(packed)
    assert torch.equal(cache(keys, packed), want), "cached and uncached outputs differ"
    no_pixels = [False] * B
    idx = torch.tensor([cache.table.present[k] for k in keys], dtype=torch.int32, device=dev)
    out = torch.empty(B, 3, 224, 224, device=dev)
    arms = {
        "GpuImageTransform (uncached)": lambda: tf(packed),
        "cache, all hit": lambda: cache(keys, None, no_pixels),
        "gather kernel": lambda: K.gather_normalize_u8(cache.storage, idx, 224, 224, MEAN, STD, out),
    }
    assert torch.equal(cache(keys, None, no_pixels), want)
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in arms}
    ev = []
    chain = graph_of(arms["gather kernel"], 10 * args.calls)
    chain.replay()
    for _ in range(args.repeats):
        for k, fn in arms.items():
            times[k].append(timed(fn, args.calls))
        ev.append(event_timed(chain, 10 * args.calls))
    moved = B * (224 * 224 * 3) * (1 + 4)
    res = {"ms_per_call": {k: summary(v) for k, v in times.items()},
           "gather_kernel_ms_graph_replay": summary(ev), "gather_bytes": moved,
           "gather_TB_per_s_graph_replay": round(moved / (statistics.median(ev) * 1e-3) / 1e12, 3),
           "uploaded_bytes_uncached": int(packed.data.numel())}
    return res


def train_arm(gb, tree, dev, args):
    import checkpoint  # noqa: F401
    import dataset as D
    from models import attention as A
    from pathconf import PathConfig
    anno, img_dir, vf, vocab = tree
    PathConfig.train_anno_file, PathConfig.train_img_dir, PathConfig.vocab_file = anno, img_dir, vf
    counter = torch.zeros(args.train_workers + 1, dtype=torch.int64).share_memory_()
    marks, batches = [], []
    decode = D.COCODataset._get_transformed_img
    save, clip = A.save_checkpoint, A.clip_gradient

    def counting(self, img_id):
        info = torch.utils.data.get_worker_info()
        counter[0 if info is None else info.id + 1] += 1  # one cell per worker: no two processes share one
        return decode(self, img_id)

    def epoch_end(*a, **k):
        torch.cuda.synchronize()
        marks.append((time.perf_counter(), int(counter.sum())))

    def batch_start(*a, **k):  # train() clips once per batch, as soon as the loader has delivered it
        batches.append(time.perf_counter())
        return clip(*a, **k)

    D.COCODataset._get_transformed_img = counting
    A.save_checkpoint, A.clip_gradient = epoch_end, batch_start
    try:
        a = types.SimpleNamespace(
            model_name=f"imagepipe_bench_{gb}", model="attention", attention_dim=512, decoder_dim=512,
            decoder_dropout=0.5, embed_size=512, epochs=2, batch_size=64, workers=args.train_workers, encoder_lr=1e-4,
            decoder_lr=1e-4, grad_clip=5.0, alpha_c=1.0, fine_tune_encoder=False, fine_tune_embedding=False,
            checkpoint=None, print_freq=args.print_freq, use_glove=False, max_caption_length=-1, use_bert=False, synthetic=False,
            synthetic_size=0, vocab_size=len(vocab), trusted_checkpoint=False, image_cache_gb=gb)
        torch.manual_seed(0)
        t0 = time.perf_counter()
        A.train(dev, a)
    finally:
        D.COCODataset._get_transformed_img = decode
        A.save_checkpoint, A.clip_gradient = save, clip
    n = 5 * args.train_images
    epochs, prev_t, prev_c = [], t0, 0
    for t, c in marks:
        first = min(b for b in batches if b > prev_t)  # the epoch's first batch: its loader workers are up
        epochs.append({"images_per_s": round(n / (t - prev_t), 1), "seconds": round(t - prev_t, 3),
                       "seconds_to_first_batch": round(first - prev_t, 3),
                       "images_per_s_after_first_batch": round((n - 64) / (t - first), 1), "decodes": c - prev_c})
        prev_t, prev_c = t, c
    cache = A.train.last_image_cache
    return {"epochs": epochs, "cache_stats": None if cache is None else dict(cache.stats),
            "step_counts": dict(A.train.last_step.counts)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--train-workers", type=int, default=12,
                    help="loader workers of arm (c); they are forked from the process that holds the device")
    ap.add_argument("--print-freq", type=int, default=1000, help="train(): batches between device synchronisations")
    ap.add_argument("--train-images", type=int, default=512)
    ap.add_argument("--decode-passes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-train", action="store_true", help="skip arm (c)")
    ap.add_argument("--train-arm", nargs=2, metavar=("GB", "TREE"), default=None,
                    help="(internal) run one train() arm over the tree at TREE and print its JSON")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.train_arm is not None:
        root = args.train_arm[1]
        with open(os.path.join(root, "vocab.pkl"), "rb") as f:
            vocab = pickle.load(f)
        tree = (os.path.join(root, "captions.json"), os.path.join(root, "images"), os.path.join(root, "vocab.pkl"), vocab)
        print(json.dumps(train_arm(float(args.train_arm[0]), tree, torch.device("cuda"), args)))
        return
    res = {"workers": args.workers, "train_workers": args.train_workers, "train_images": args.train_images}
    with tempfile.TemporaryDirectory(prefix="imagepipe_bench_") as root:
        tree = write_tree(root, args.train_images)
        paths = sorted(os.path.join(tree[1], f) for f in os.listdir(tree[1]))
        res["jpeg_bytes_mean"] = int(np.mean([os.path.getsize(p) for p in paths]))
        # arm (a) first: host only, before this process opens the device
        res["decode_only_images_per_s"] = {str(w): round(decode_rate(paths, w, args.decode_passes), 1)
                                           for w in (1, args.workers)}
        print(json.dumps({"arm": "decode only", "images_per_s": res["decode_only_images_per_s"]}), flush=True)
        if not torch.cuda.is_available():
            raise SystemExit("imagepipe_bench needs the GPU (no fallback)")
        dev = torch.device("cuda")
        res["device"] = torch.cuda.get_device_name(0)
        res["batch64"] = batch_arms(paths, dev, args)
        print(json.dumps({"arm": "batch of 64", **res["batch64"]}), flush=True)
        if not args.no_train:
            res["train"] = {}
            for gb in (0, 1.0):  # a fresh process each: neither arm inherits the other's pinned memory or graphs
                cmd = [sys.executable, os.path.abspath(__file__), "--train-arm", str(gb), root, "--train-workers",
                       str(args.train_workers), "--train-images", str(args.train_images), "--print-freq",
                       str(args.print_freq)]
                out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=root).stdout
                res["train"][f"image_cache_gb={gb:g}"] = json.loads(out.strip().splitlines()[-1])
                print(json.dumps({"arm": f"train image_cache_gb={gb:g}", **res["train"][f"image_cache_gb={gb:g}"]}),
                      flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
