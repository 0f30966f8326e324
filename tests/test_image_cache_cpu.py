"""CPU: the device image cache's host side. The two new entry points validate their arguments
before any launch (no GPU is touched), capmi.imagepipe.SlotTable follows every rule of its contract, and
COCODataset(return_image_key=True) returns keys, skips the decode of a present image and shares its flags with
DataLoader workers that were started before the flags were set."""
import ctypes

import numpy as np
import pytest
import torch

EINVAL = 1001


def test_new_entry_points_validate_before_launch():
    import capmi
    from capmi._lib import lib
    assert capmi.ABI_VERSION == 27 and lib.capmi_abi_version() == 27
    p = 256  # a non-null stand-in: validation never dereferences it
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def resize(src=p, offs=p, hs=p, ws=p, slot=p, n=1, max_h=8, max_w=8, OH=4, OW=4, tmp=p, slots=p, n_slots=2):
        return lib.capmi_resize_u8_slots(src, offs, hs, ws, slot, n, max_h, max_w, OH, OW, tmp, slots, n_slots, None)

    for name in ("src", "offs", "hs", "ws", "slot", "tmp", "slots"):
        assert resize(**{name: None}) == EINVAL, name
    for name in ("max_h", "max_w", "OH", "OW", "n_slots"):
        assert resize(**{name: 0}) == EINVAL and resize(**{name: -3}) == EINVAL, name
    assert resize(n=-1) == EINVAL
    assert resize(n=0) == 0  # nothing to do: no launch
    assert resize(max_w=4000, OW=4) == 1003  # more than 32 taps (CAPMI_ERANGE), as capmi_resize_normalize_u8

    def gather(slots=p, n_slots=2, slot=p, B=1, OH=4, OW=4, mean=m, std=m, out=p):
        return lib.capmi_gather_normalize_u8(slots, n_slots, slot, B, OH, OW, mean, std, out, None)

    for name in ("slots", "slot", "mean", "std", "out"):
        assert gather(**{name: None}) == EINVAL, name
    for name in ("n_slots", "OH", "OW"):
        assert gather(**{name: 0}) == EINVAL and gather(**{name: -1}) == EINVAL, name
    assert gather(B=-1) == EINVAL
    assert gather(B=0) == 0
    assert gather(B=65536) == 1003


def test_kernel_wrappers_need_device_tensors():
    from capmi import kernels as K
    u8 = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        K.gather_normalize_u8(u8, torch.zeros(1, dtype=torch.int32), 4, 4, (0, 0, 0), (1, 1, 1), torch.zeros(1, 3, 4, 4))


# ---------------------------------------------------------------------------------------------------
# SlotTable
# ---------------------------------------------------------------------------------------------------
def test_slot_table_insert_then_hit():
    from capmi.imagepipe import SlotTable
    t = SlotTable(4, 2)
    gather, resample, inserted = t.assign([7, 3], [True, True])
    assert gather == [0, 1] and resample == [(0, 0), (1, 1)] and inserted == [7, 3]
    assert t.present == {7: 0, 3: 1}
    assert t.stats == dict(hits=0, inserted=2, passthrough=0, stale_pixels=0, resampled=2)
    gather, resample, inserted = t.assign([3, 7, 3], [False, False, False])  # all hits, no pixels needed
    assert gather == [1, 0, 1] and resample == [] and inserted == []
    assert t.stats == dict(hits=3, inserted=2, passthrough=0, stale_pixels=0, resampled=2)


def test_slot_table_duplicate_new_key_is_resampled_once():
    from capmi.imagepipe import SlotTable
    t = SlotTable(4, 2)
    gather, resample, inserted = t.assign([5, 9, 5], [True, True, True])
    assert gather == [0, 1, 0] and resample == [(0, 0), (1, 1)] and inserted == [5, 9]
    assert t.stats["resampled"] == 2 and t.stats["inserted"] == 2 and t.stats["hits"] == 1
    assert t.stats["stale_pixels"] == 0  # the key was not present when its second copy was decoded


def test_slot_table_full_uses_scratch_and_forgets():
    from capmi.imagepipe import SlotTable
    t = SlotTable(2, 3)
    t.assign([1, 2], [True, True])
    gather, resample, inserted = t.assign([2, 8, 9, 8], [False, True, True, True])
    assert gather == [1, 2, 3, 2]  # scratch slots start at capacity; the repeated key shares one
    assert resample == [(1, 2), (2, 3)] and inserted == []
    assert t.present == {1: 0, 2: 1}  # never marked present
    assert t.stats == dict(hits=2, inserted=2, passthrough=2, stale_pixels=0, resampled=4)
    # the same key is a miss again in the next call, and scratch slots are handed out from the start again
    gather, resample, _ = t.assign([9], [True])
    assert gather == [2] and resample == [(0, 2)] and t.stats["passthrough"] == 3
    with pytest.raises(KeyError):
        t.assign([9], [False])


def test_slot_table_partly_full_batch():
    from capmi.imagepipe import SlotTable
    t = SlotTable(3, 2)
    gather, resample, inserted = t.assign([10, 11, 12, 13], [True] * 4)  # three fit, the fourth passes through
    assert gather == [0, 1, 2, 3] and inserted == [10, 11, 12] and len(resample) == 4
    assert t.stats["inserted"] == 3 and t.stats["passthrough"] == 1 and len(t.present) == 3


def test_slot_table_stale_pixels_are_counted_and_ignored():
    from capmi.imagepipe import SlotTable
    t = SlotTable(4, 2)
    t.assign([4], [True])
    gather, resample, inserted = t.assign([4, 6], [True, True])  # a worker decoded 4 before it saw the flag
    assert gather == [0, 1] and resample == [(1, 1)] and inserted == [6]
    assert t.stats == dict(hits=1, inserted=2, passthrough=0, stale_pixels=1, resampled=2)


def test_slot_table_errors_change_nothing():
    from capmi.imagepipe import SlotTable
    t = SlotTable(1, 1)
    with pytest.raises(KeyError):
        t.assign([3, 4], [True, False])  # 4: not present, no pixels
    assert t.present == {} and not any(t.stats.values())
    t.assign([3], [True])
    with pytest.raises(ValueError):
        t.assign([5, 6], [True, True])  # two pass-through items, one scratch slot
    assert t.present == {3: 0} and t.stats == dict(hits=0, inserted=1, passthrough=0, stale_pixels=0, resampled=1)
    with pytest.raises(ValueError):
        t.assign([1, 2], [True])


def test_from_gb_capacity():
    """min(n_images, floor(gb * 2^30 / slot bytes)): the storage shape is all that is checked here (meta device)."""
    from capmi.imagepipe import DeviceImageCache
    slot = 224 * 224 * 3
    c = DeviceImageCache.from_gb("meta", 1.0, 82783, 64)
    assert c.table.capacity == 2 ** 30 // slot == 7133 and tuple(c.storage.shape) == (7133 + 64, 224, 224, 3)
    assert DeviceImageCache.from_gb("meta", 13.0, 82783, 64).table.capacity == 82783
    assert DeviceImageCache.from_gb("meta", 1e-4, 10, 4, size=(5, 7)).table.capacity == 10


# ---------------------------------------------------------------------------------------------------
# dataset protocol
# ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def coco(tmp_path, monkeypatch):
    from pathconf import PathConfig
    from test_data_cpu import make_coco
    anno, img_dir, vocab = make_coco(tmp_path, n_img=4, sizes=((48, 64), (37, 50), (24, 24)))
    monkeypatch.setattr(PathConfig, "train_anno_file", str(anno))
    monkeypatch.setattr(PathConfig, "train_img_dir", str(img_dir))
    monkeypatch.setattr(PathConfig, "val_anno_file", str(anno))
    monkeypatch.setattr(PathConfig, "val_img_dir", str(img_dir))
    return vocab


def test_dataset_default_items_unchanged(coco):
    from dataset import COCODataset
    ds = COCODataset("train", caption_max_len=-1, vocab=coco)
    item = ds[2]
    assert len(item) == 2 and isinstance(item[0], np.ndarray) and item[0].shape == (37, 50, 3)
    assert not ds.return_image_key and not hasattr(ds, "present")
    # keys are a train-mode, no-transform protocol: elsewhere the flag changes nothing
    assert len(COCODataset("val", caption_max_len=-1, vocab=coco, return_image_key=True)[0]) == 4
    t = COCODataset("train", img_transform=lambda im: im.size, caption_max_len=-1, vocab=coco, return_image_key=True)
    assert len(t[0]) == 2 and t[0][0] == (64, 48)


def test_dataset_keys_and_present_flags(coco):
    from dataset import COCODataset
    plain = COCODataset("train", caption_max_len=-1, vocab=coco)
    ds = COCODataset("train", caption_max_len=-1, vocab=coco, return_image_key=True)
    assert ds.present.dtype == torch.uint8 and ds.present.numel() == len(ds.img_ids) == 4 and ds.present.is_shared()
    assert len(ds) == len(plain) == 8
    for i in range(len(ds)):
        img, cap, key = ds[i]
        assert ds.img_ids[key] == ds.caption_img_mappings[i]["img_id"]
        assert np.array_equal(img, plain[i][0]) and torch.equal(cap, plain[i][1])
    ds.present[1] = 1
    for i in range(len(ds)):
        img, cap, key = ds[i]
        assert (img is None) == (key == 1) and torch.equal(cap, plain[i][1])


def test_workers_see_flags_set_after_they_started(coco):
    """Shared-memory visibility: persistent workers forked before any flag is set return no pixels in a second
    pass, after the main process has set every flag."""
    from capmi.imagepipe import KeyedImages
    from dataset import COCODataset
    ds = COCODataset("train", caption_max_len=-1, vocab=coco, return_image_key=True)

    def collate(data):
        imgs, caps, keys = zip(*data)
        return KeyedImages(imgs, keys)

    loader = torch.utils.data.DataLoader(ds, batch_size=3, num_workers=2, collate_fn=collate, persistent_workers=True)
    first = list(loader)  # the workers exist from here on
    assert sum(sum(b.has_pixels) for b in first) == 8 and sum(len(b.packed) for b in first) == 8
    ds.present[:] = 1
    second = list(loader)
    assert sorted(k for b in second for k in b.keys) == sorted(k for b in first for k in b.keys)
    assert sum(sum(b.has_pixels) for b in second) == 0 and all(len(b.packed) == 0 for b in second)
    del loader


def test_keyed_images_packs_only_decoded_items():
    from capmi.imagepipe import KeyedImages, collate_images
    a = np.full((2, 3, 3), 7, np.uint8)
    b = collate_images((a, None, a), (4, 5, 4))
    assert isinstance(b, KeyedImages) and len(b) == 3 and b.keys == [4, 5, 4] and b.has_pixels == [True, False, True]
    assert len(b.packed) == 2 and b.packed.data.numel() == 36
    t = collate_images((torch.zeros(3, 2, 2), torch.ones(3, 2, 2)))
    assert isinstance(t, torch.Tensor) and t.shape == (2, 3, 2, 2)


def test_train_cli_flag():
    from train import parse_args
    assert parse_args(["x", "--model", "attention"]).image_cache_gb == 0
    assert parse_args(["x", "--model", "attention", "--image_cache_gb", "12.5"]).image_cache_gb == 12.5
    import types
    from capmi.imagepipe import image_cache_requested
    assert not image_cache_requested(types.SimpleNamespace(), "cuda")  # args built by hand: no attribute
    assert not image_cache_requested(types.SimpleNamespace(image_cache_gb=1.0), "cpu")
    assert image_cache_requested(types.SimpleNamespace(image_cache_gb=1.0), torch.device("cuda", 0))
