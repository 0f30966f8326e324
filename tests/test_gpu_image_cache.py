"""GPU: the device image cache (capmi.imagepipe.DeviceImageCache over capmi_resize_u8_slots and
capmi_gather_normalize_u8). Everything is exact: the cached path returns the bits of the uncached
GpuImageTransform (itself pinned to Pillow by tests/test_gpu_image.py), each slot holds Pillow's uint8 resample,
a full cache passes images through scratch slots without touching a permanent one, the gather is right at
shapes on both of its kernels with nothing written around its output, and train() with the cache logs the
losses of train() without it."""
import pickle
import types

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(480, 640), (375, 500), (224, 224), (100, 150), (333, 251), (1000, 90), (17, 300)]  # tests/test_gpu_image.py


@pytest.fixture(scope="module")
def images():
    """The arrays, and what the uncached path makes of them (computed once, never modified)."""
    from capmi.imagepipe import GpuImageTransform, PackedImages
    rng = np.random.default_rng(3)
    arrs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    want = GpuImageTransform(DEV)(PackedImages(arrs))
    torch.cuda.synchronize()
    return arrs, want


def _packed(arrs, idx):
    from capmi.imagepipe import PackedImages
    return PackedImages([arrs[i] for i in idx])


def test_cached_path_equals_uncached_bit_for_bit(images):
    from capmi.imagepipe import DeviceImageCache
    arrs, want = images
    n = len(arrs)
    cache = DeviceImageCache(DEV, 10, n)
    cache.storage.fill_(0xA5)
    keys = [100 + i for i in range(n)]
    # all miss
    out = cache(keys, _packed(arrs, range(n)))
    assert torch.equal(out, want)
    assert cache.stats == dict(hits=0, inserted=n, passthrough=0, stale_pixels=0, resampled=n)
    # each slot is Pillow's resample, byte for byte
    slots = cache.storage.cpu().numpy()
    for i, a in enumerate(arrs):
        pil = np.asarray(Image.fromarray(a).resize((224, 224), Image.BILINEAR))
        assert np.array_equal(slots[cache.table.present[keys[i]]], pil), SIZES[i]
    # permanent slots never assigned, and the scratch slots, were not written
    assert bool((cache.storage[n:] == 0xA5).all())
    # all hit, no pixels: permuted, two keys repeated
    order = [4, 0, 6, 2, 2, 5, 0]
    out = cache([keys[i] for i in order], None, [False] * len(order))
    assert torch.equal(out, want[order])
    assert cache.stats["hits"] == len(order) and cache.stats["resampled"] == n


def test_mixed_hits_and_misses(images):
    from capmi.imagepipe import DeviceImageCache
    arrs, want = images
    cache = DeviceImageCache(DEV, 10, 8)
    assert torch.equal(cache([0, 3, 5], _packed(arrs, [0, 3, 5])), want[[0, 3, 5]])
    # 3 and 0 hit (0 comes with stale pixels), 1 and 6 miss, 6 twice (both copies decoded), 5 hits without pixels
    keys, has = [3, 1, 0, 6, 5, 6], [False, True, True, True, False, True]
    out = cache(keys, _packed(arrs, [1, 0, 6, 6]), has)
    assert torch.equal(out, want[keys])
    assert cache.stats == dict(hits=4, inserted=5, passthrough=0, stale_pixels=1, resampled=5)
    with pytest.raises(KeyError):
        cache([2], None, [False])
    with pytest.raises(ValueError):
        cache([2, 4], _packed(arrs, [2]), [True, True])  # packed must hold exactly the flagged items


def test_full_cache_passes_through_scratch_slots(images):
    from capmi.imagepipe import DeviceImageCache
    arrs, want = images
    cache = DeviceImageCache(DEV, 2, 3)
    cache.storage.fill_(0xA5)
    assert torch.equal(cache([0, 1, 2], _packed(arrs, [0, 1, 2])), want[:3])  # 2 passes through
    kept = cache.storage[:2].clone()
    assert torch.equal(cache([3, 0, 4, 3], _packed(arrs, [3, 4, 3]), [True, False, True, True]), want[[3, 0, 4, 3]])
    assert len(cache.table.present) == 2 and sorted(cache.table.present) == [0, 1]
    assert cache.stats == dict(hits=2, inserted=2, passthrough=3, stale_pixels=0, resampled=5)
    assert torch.equal(cache.storage[:2], kept)  # permanent slots untouched by pass-through images
    assert bool((cache.storage[4] == 0xA5).all())  # the third scratch slot was never needed
    assert torch.equal(cache([2], _packed(arrs, [2])), want[2:3])  # a miss again


def test_present_flags_are_set_for_inserted_keys_only(images):
    from capmi.imagepipe import DeviceImageCache
    arrs, want = images
    present = torch.zeros(9, dtype=torch.uint8).share_memory_()
    cache = DeviceImageCache(DEV, 2, 4, present=present)
    cache([8, 3, 5], _packed(arrs, [0, 3, 5]))
    assert present.tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 1]  # 5 passed through: a worker must decode it again


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", [(5, 7), (1, 1), (3, 4), (224, 224)])
def test_gather_edge_shapes(size, B):
    """(5, 7) and (1, 1): one pixel per lane; (3, 4) and (224, 224): four pixels per lane, (224, 224) over many
    blocks. The output sits inside a NaN-filled buffer whose margins must stay NaN; slots repeat and are not in
    order."""
    from capmi import kernels as K
    from capmi.imagepipe import MEAN, STD
    OH, OW = size
    rng = np.random.default_rng(OH * 1000 + OW)
    n_slots = 5
    slots = rng.integers(0, 256, (n_slots, OH, OW, 3), dtype=np.uint8)
    idx = [4, 1, 4][:B]
    n = B * 3 * OH * OW
    buf = torch.full((n + 64,), float("nan"), device=DEV)
    out = buf[32:32 + n].view(B, 3, OH, OW)  # 128 B into the allocation: 16-B aligned
    K.gather_normalize_u8(torch.from_numpy(slots).to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), OH, OW,
                          MEAN, STD, out)
    torch.cuda.synchronize()
    m = np.array(MEAN, np.float32).reshape(1, 1, 3)
    s = np.array(STD, np.float32).reshape(1, 1, 3)
    want = np.stack([((slots[i].astype(np.float32) / np.float32(255) - m) / s).transpose(2, 0, 1) for i in idx])
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool(torch.isnan(buf[:32]).all()) and bool(torch.isnan(buf[32 + n:]).all())


def test_gather_into_a_misaligned_output():
    """An output 4 B off a 16-B boundary takes the one-pixel kernel at a shape the four-pixel one would take."""
    from capmi import kernels as K
    from capmi.imagepipe import MEAN, STD
    OH, OW, B = 6, 8, 2
    rng = np.random.default_rng(11)
    slots = rng.integers(0, 256, (3, OH, OW, 3), dtype=np.uint8)
    n = B * 3 * OH * OW
    buf = torch.full((n + 64,), float("nan"), device=DEV)
    out = buf[33:33 + n].view(B, 3, OH, OW)
    K.gather_normalize_u8(torch.from_numpy(slots).to(DEV), torch.tensor([2, 0], dtype=torch.int32, device=DEV), OH, OW,
                          MEAN, STD, out)
    torch.cuda.synchronize()
    m = np.array(MEAN, np.float32).reshape(1, 1, 3)
    s = np.array(STD, np.float32).reshape(1, 1, 3)
    want = np.stack([((slots[i].astype(np.float32) / np.float32(255) - m) / s).transpose(2, 0, 1) for i in (2, 0)])
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool(torch.isnan(buf[:33]).all()) and bool(torch.isnan(buf[33 + n:]).all())


def test_slot_outside_the_storage_never_reaches_the_kernel(monkeypatch):
    from capmi import kernels as K
    from capmi.imagepipe import DeviceImageCache
    cache = DeviceImageCache(DEV, 2, 1, size=(3, 4))
    calls = []
    monkeypatch.setattr(K, "gather_normalize_u8", lambda *a, **k: calls.append(a))
    for bad in ([3], [0, -1], [2 ** 31]):
        with pytest.raises(ValueError):
            cache.gather(bad)
    assert calls == []
    cache.gather([2, 0])  # the last slot of the storage is fine
    assert len(calls) == 1


# ---------------------------------------------------------------------------------------------------
# train()
# ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def coco_tree(tmp_path, monkeypatch):
    import checkpoint as C
    from pathconf import PathConfig
    from test_data_cpu import make_coco
    anno, img_dir, vocab = make_coco(tmp_path, n_img=4)
    vf = tmp_path / "vocab.pkl"
    with open(vf, "wb") as f:
        pickle.dump(vocab, f)
    monkeypatch.setattr(PathConfig, "train_anno_file", str(anno))
    monkeypatch.setattr(PathConfig, "train_img_dir", str(img_dir))
    monkeypatch.setattr(PathConfig, "vocab_file", str(vf))
    monkeypatch.setattr(C, "CHECKPOINTS_DIR", str(tmp_path / "ck"))
    return tmp_path, vocab


def _args(name, vocab, gb):
    return types.SimpleNamespace(
        model_name=name, model="attention", attention_dim=64, decoder_dim=64, decoder_dropout=0.5, embed_size=32,
        epochs=2, batch_size=4, workers=0, encoder_lr=1e-4, decoder_lr=1e-4, grad_clip=5.0, alpha_c=1.0,
        fine_tune_encoder=False, fine_tune_embedding=False, checkpoint=None, print_freq=1, use_glove=False,
        max_caption_length=-1, use_bert=False, synthetic=False, synthetic_size=0, vocab_size=len(vocab),
        trusted_checkpoint=False, image_cache_gb=gb)


def test_attention_train_with_the_cache_equals_without(coco_tree):
    """4 images x 2 captions, batch 4, two epochs: every image is resampled once (4), every other item is a hit
    (16 - 4 = 12: a second caption of a new image in the same batch, and all of epoch 2, which decodes nothing),
    and the losses are those of the uncached run, bit for bit."""
    from models import attention as A
    tmp_path, vocab = coco_tree
    losses = {}
    for gb in (0, 1.0):
        torch.manual_seed(0)
        A.train(torch.device(DEV), _args(f"cache{gb}", vocab, gb))
        ck = torch.load(tmp_path / "ck" / f"cache{gb}_1.pth.tar", weights_only=True)
        losses[gb] = ck["metrics"]["epoch_losses"]
        cache = A.train.last_image_cache
        assert (cache is None) == (gb == 0)
    assert [len(e) for e in losses[0]] == [2, 2] and np.isfinite(np.array(losses[0])).all()
    print("losses without / with the cache:", losses[0], losses[1.0])
    np.testing.assert_array_equal(np.array(losses[1.0]), np.array(losses[0]))
    st = cache.stats
    assert st["resampled"] == 4 and st["hits"] == 12 and st["stale_pixels"] == 0, st
    assert st["inserted"] == 4 and st["passthrough"] == 0 and len(cache.table.present) == 4


def test_step_capture_beside_a_thread_that_pins_memory():
    """What train() meets with loader workers: the DataLoader's pin-memory thread allocates pinned host memory
    while a step is being captured. In the "thread_local" capture mode train() then selects, the capture survives
    it (in the default "global" mode the runtime invalidates it). The thread here allocates as that one does,
    holding what it allocated so that every call reaches the runtime; no processes are started."""
    import threading
    import gen
    from helpers import t
    from test_gpu_train_step import _setup
    B, L, V = 4, 7, 50
    imgs, caps = t(gen.images(5, B, 64, 64), DEV), t(gen.captions(5, B, L, V), DEV)
    enc, dec, opt, Step = _setup(0.0)
    step = Step(enc, dec, opt, alpha_c=1.0, graph=True, seed=123)
    assert step.capture_error_mode == "global"
    step.capture_error_mode = "thread_local"
    stop, held = threading.Event(), []

    def pin():
        while not stop.is_set() and len(held) < 2000:  # at most 125 MB
            held.append(torch.empty(1 << 16, dtype=torch.uint8).pin_memory())

    th = threading.Thread(target=pin)
    th.start()
    try:
        losses = [float(step(imgs, caps, [L] * B)) for _ in range(3)]
        torch.cuda.synchronize()
    finally:
        stop.set()
        th.join()
    assert step.counts["capture"] == 1 and step.counts["replay"] == 3 and np.isfinite(losses).all(), (step.counts, losses)
    assert len(held) > 0


class TinyEncoder(torch.nn.Module):
    """Stands for models.encoder.Encoder in the baseline's train(), as in tests/test_gpu_baseline_train_step.py:
    the image's channel means through the embed Linear (the loss still depends on every pixel)."""

    def __init__(self, embed_size):
        super().__init__()
        self.embed = torch.nn.Linear(3, embed_size)

    def forward(self, imgs):
        return self.embed(imgs.mean((2, 3)))


def test_baseline_train_on_real_coco_with_and_without_the_cache(coco_tree, monkeypatch):
    import models.baseline as MB
    tmp_path, vocab = coco_tree
    monkeypatch.setattr(MB, "Encoder", TinyEncoder)
    monkeypatch.delenv("CAPMI_BASELINE_STEP", raising=False)
    losses = {}
    for gb in (0, 1.0):
        args = _args(f"base{gb}", vocab, gb)
        args.model, args.decoder_dim, args.embed_size = "baseline", 24, 16
        torch.manual_seed(0)
        MB.train(torch.device(DEV), args)
        ck = torch.load(tmp_path / "ck" / f"base{gb}_1.pth.tar", weights_only=True)
        losses[gb] = ck["metrics"]["epoch_losses"]
        assert (MB.train.last_image_cache is None) == (gb == 0)
    assert [len(e) for e in losses[0]] == [2, 2] and np.isfinite(np.array(losses[0])).all(), losses[0]
    np.testing.assert_array_equal(np.array(losses[1.0]), np.array(losses[0]))
    st = MB.train.last_image_cache.stats
    assert st["resampled"] == 4 and st["hits"] == 12 and st["stale_pixels"] == 0, st
