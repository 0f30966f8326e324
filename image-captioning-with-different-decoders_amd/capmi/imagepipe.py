"""The reference's image transform on the GPU.

Reference (models/attention.py:296-301 + dataset.py:55-59): every DataLoader worker decodes a
JPEG, applies Resize((224, 224)) -> ToTensor -> Normalize on the CPU and the collate stacks
(B, 3, 224, 224) fp32. Here the workers only decode (PIL) and the collate packs the uint8 RGB
pixels of the batch into one (pinned) buffer; on the device ``GpuImageTransform`` runs
``capmi_resize_normalize_u8`` (csrc/image.hip): the same resample, bit-identical to Pillow's,
then ToTensor + Normalize. The host keeps only the JPEG decode: resampling a 640x480 image and
normalising it costs the CPU several ms, which at ~4000 training images/s per GPU would take tens
of cores. PCIe then carries the decoded uint8 pixels (0.92 MB for 640x480, ~1.5x the 0.6 MB fp32
tensor the reference copies; 3.7 GB/s at that rate).

``DeviceImageCache`` (train.py --image_cache_gb) goes one step further: the transform is deterministic, so the
resized uint8 image of every picture stays on the device, each JPEG is decoded once per run, and a batch of
cached images is one gather kernel (``capmi_gather_normalize_u8``) with the same output bits.
"""
import numpy as np
import torch

from . import kernels as K

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


class PackedImages:
    """A batch of decoded RGB images, uint8 HWC, packed back to back (the collate's output)."""

    def __init__(self, arrays, pin=True):
        sizes = [a.shape[0] * a.shape[1] * 3 for a in arrays]
        self.heights = torch.tensor([a.shape[0] for a in arrays], dtype=torch.int32)
        self.widths = torch.tensor([a.shape[1] for a in arrays], dtype=torch.int32)
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]) if arrays else [],
                                    dtype=torch.int64)
        buf = torch.empty(int(sum(sizes)), dtype=torch.uint8)
        o = 0
        for a, n in zip(arrays, sizes):
            if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                raise ValueError("PackedImages takes (H, W, 3) uint8 arrays")
            buf[o:o + n] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
            o += n
        self.data = buf.pin_memory() if pin and torch.cuda.is_available() else buf

    def __len__(self):
        return int(self.heights.numel())

    def pin_memory(self):  # DataLoader(pin_memory=True) calls this on custom batch types
        if not self.data.is_pinned():
            self.data = self.data.pin_memory()
        return self


class GpuImageTransform:
    """PackedImages -> (B, 3, OH, OW) fp32 on `device`: Resize (PIL bilinear, bit-exact) +
    ToTensor + Normalize(MEAN, STD). Workspaces grow to the largest batch seen and are reused."""

    def __init__(self, device, size=(224, 224), mean=MEAN, std=STD):
        self.device = torch.device(device)
        self.size = tuple(size)
        self.mean, self.std = tuple(mean), tuple(std)
        self._tmp = None

    def __call__(self, batch: PackedImages):
        dev = self.device
        B = len(batch)
        OH, OW = self.size
        out = torch.empty(B, 3, OH, OW, device=dev, dtype=torch.float32)
        if B == 0:
            return out
        max_h, max_w = int(batch.heights.max()), int(batch.widths.max())
        src = batch.data.to(dev, non_blocking=True)
        offs = batch.offsets.to(dev, non_blocking=True)
        hs = batch.heights.to(dev, non_blocking=True)
        ws = batch.widths.to(dev, non_blocking=True)
        need = B * max_h * OW * 3
        if self._tmp is None or self._tmp.numel() < need:
            self._tmp = torch.empty(need, device=dev, dtype=torch.uint8)
        K.resize_normalize_u8(src, offs, hs, ws, max_h, max_w, OH, OW, self.mean, self.std, self._tmp, out)
        return out


class SlotTable:
    """Host bookkeeping of the device image cache (no device memory): image key -> permanent slot in
    [0, capacity). Nothing is ever evicted: an epoch visits the images in a random permutation, so LRU would
    thrash, and "present is never cleared" is what lets loader workers skip the decode of a present key without
    a race. Per call there are `scratch` more slots [capacity, capacity + scratch) for images that found the
    table full: resampled, used by that call and forgotten."""

    def __init__(self, capacity, scratch):
        if capacity < 0 or scratch < 0:
            raise ValueError("SlotTable: capacity and scratch must be >= 0")
        self.capacity, self.scratch = int(capacity), int(scratch)
        self.present = {}  # key -> permanent slot
        self.stats = dict(hits=0, inserted=0, passthrough=0, stale_pixels=0, resampled=0)

    def assign(self, keys, has_pixels):
        """One batch. Returns (gather, resample, inserted): gather[i] = the slot batch item i reads; resample =
        [(i, slot)], the items whose pixels are to be resampled into `slot` first; inserted = the keys that took
        a permanent slot in this call. A present key is a hit, and pixels that came with it are ignored (counted
        as stale_pixels: a worker decoded before the insert was visible to it). A new key with pixels takes the
        next permanent slot, or a scratch slot once the table is full; a later item of the batch with the same
        key reads that slot (a hit). A new key without pixels raises KeyError. Nothing changes when it raises."""
        if len(keys) != len(has_pixels):
            raise ValueError("SlotTable.assign: one has_pixels flag per key")
        gather, resample, inserted = [], [], []
        new = {}  # keys first seen in this call -> slot
        st = dict.fromkeys(self.stats, 0)
        n_perm, n_scratch = len(self.present), 0
        for i, (key, pix) in enumerate(zip(keys, has_pixels)):
            key = int(key)
            if key in self.present:
                st["hits"] += 1
                st["stale_pixels"] += bool(pix)
                gather.append(self.present[key])
            elif key in new:
                st["hits"] += 1
                gather.append(new[key])
            elif not pix:
                raise KeyError(f"image {key} is not cached and came without pixels")
            else:
                if n_perm < self.capacity:
                    slot, n_perm = n_perm, n_perm + 1
                    inserted.append(key)
                    st["inserted"] += 1
                elif n_scratch < self.scratch:
                    slot, n_scratch = self.capacity + n_scratch, n_scratch + 1
                    st["passthrough"] += 1
                else:
                    raise ValueError(f"more than {self.scratch} uncached images in one batch of a full cache")
                new[key] = slot
                resample.append((i, slot))
                st["resampled"] += 1
                gather.append(slot)
        for key in inserted:
            self.present[key] = new[key]
        for k, v in st.items():
            self.stats[k] += v
        return gather, resample, inserted


class DeviceImageCache:
    """The resized uint8 image of every picture seen, kept on `device`: one uint8 tensor of
    (capacity_images + max_batch, OH, OW, 3), a SlotTable over it and the resample workspace. The reference's
    transform is deterministic, so a JPEG needs decoding once per run: a new image is resampled into its slot
    (capmi_resize_u8_slots, the bytes GpuImageTransform would normalise), and every batch is one gather
    (capmi_gather_normalize_u8) whose output is bit-equal to GpuImageTransform's.

    `present`: the dataset's shared uint8 flag array (COCODataset(return_image_key=True).present); a key is
    flagged there only after its insert has been issued, so a worker that sees the flag may skip the decode."""

    def __init__(self, device, capacity_images, max_batch, size=(224, 224), mean=MEAN, std=STD, present=None):
        self.device = torch.device(device)
        self.size = tuple(size)
        self.mean, self.std = tuple(mean), tuple(std)
        self.table = SlotTable(capacity_images, max_batch)
        self.stats = self.table.stats
        OH, OW = self.size
        self.storage = torch.empty(int(capacity_images) + int(max_batch), OH, OW, 3, device=self.device,
                                   dtype=torch.uint8)
        self.present = present
        self._tmp = None

    @classmethod
    def from_gb(cls, device, gb, n_images, max_batch, size=(224, 224), **kw):
        """Capacity min(n_images, floor(gb * 2^30 / slot bytes)); the max_batch scratch slots come on top."""
        slot_bytes = size[0] * size[1] * 3
        return cls(device, min(int(n_images), int(gb * 2 ** 30 // slot_bytes)), max_batch, size=size, **kw)

    def _slots_to_device(self, idx):
        """Host slot indices -> int32 device tensor, checked against the storage first: the kernels cannot be
        told about a bad index (they skip it), so it never leaves the host. Pinned source, asynchronous copy."""
        n_slots = self.storage.shape[0]
        for s in idx:
            if not 0 <= int(s) < n_slots:
                raise ValueError(f"slot {s} outside the cache's storage [0, {n_slots})")
        return torch.tensor([int(s) for s in idx], dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)

    def gather(self, idx):
        """(len(idx), 3, OH, OW) fp32: ToTensor + Normalize of the slots `idx` (host ints), on the current stream."""
        OH, OW = self.size
        out = torch.empty(len(idx), 3, OH, OW, device=self.device, dtype=torch.float32)
        if len(idx):
            K.gather_normalize_u8(self.storage, self._slots_to_device(idx), OH, OW, self.mean, self.std, out)
        return out

    def __call__(self, keys, packed=None, has_pixels=None):
        """keys: the image key of every batch item; packed: PackedImages of only the items that carry pixels,
        in batch order; has_pixels: which items those are (default: all of them when `packed` is given)."""
        n_pix = 0 if packed is None else len(packed)
        if has_pixels is None:
            has_pixels = [packed is not None] * len(keys)
        if sum(bool(p) for p in has_pixels) != n_pix:
            raise ValueError("DeviceImageCache: `packed` must hold exactly the items flagged in has_pixels")
        gather, resample, inserted = self.table.assign(keys, has_pixels)
        if resample:
            at = np.cumsum([bool(p) for p in has_pixels]) - 1  # batch item -> its image in `packed`
            sel = torch.tensor([int(at[i]) for i, _ in resample], dtype=torch.int64)
            hs, ws = packed.heights[sel], packed.widths[sel]
            max_h, max_w = int(hs.max()), int(ws.max())
            dev = self.device
            OH, OW = self.size
            need = len(resample) * max_h * OW * 3
            if self._tmp is None or self._tmp.numel() < need:
                self._tmp = torch.empty(need, device=dev, dtype=torch.uint8)
            K.resize_u8_slots(packed.data.to(dev, non_blocking=True), packed.offsets[sel].to(dev, non_blocking=True),
                              hs.to(dev, non_blocking=True), ws.to(dev, non_blocking=True),
                              self._slots_to_device([s for _, s in resample]), max_h, max_w, OH, OW, self._tmp,
                              self.storage)
        if self.present is not None and inserted:
            self.present[torch.tensor(inserted, dtype=torch.int64)] = 1  # only now: the insert is on the stream
        return self.gather(gather)


class KeyedImages:
    """Collate output of a dataset that returns image keys (COCODataset(return_image_key=True)): the
    PackedImages of the items that were decoded, every item's key, and which items have pixels."""

    def __init__(self, imgs, keys):
        self.keys = [int(k) for k in keys]
        self.has_pixels = [im is not None for im in imgs]
        self.packed = PackedImages([im for im in imgs if im is not None], pin=False)

    def __len__(self):
        return len(self.keys)

    def pin_memory(self):
        if self.packed.data.numel():
            self.packed.pin_memory()
        return self


def collate_images(imgs, keys=None):
    """The image column of a batch: tensors are stacked (a transform ran in the workers, or synthetic data),
    decoded uint8 arrays are packed for the GPU transform, with their keys when the dataset returns them."""
    if keys is not None:
        return KeyedImages(imgs, keys)
    if isinstance(imgs[0], torch.Tensor):
        return torch.stack(imgs, dim=0)
    return PackedImages(list(imgs), pin=False)


class ImageFeeder:
    """What a training loop does with collate_images' output: a tensor is copied to `device`, PackedImages go
    through GpuImageTransform, KeyedImages through `cache` (a DeviceImageCache)."""

    def __init__(self, device, cache=None):
        self.device = torch.device(device)
        self.cache = cache
        self._tf = None

    def __call__(self, imgs):
        if isinstance(imgs, torch.Tensor):
            return imgs.to(self.device, non_blocking=True)
        if isinstance(imgs, KeyedImages):
            if self.cache is None:
                raise RuntimeError("a batch with image keys needs a DeviceImageCache")
            return self.cache(imgs.keys, imgs.packed, imgs.has_pixels)
        if self._tf is None:
            self._tf = GpuImageTransform(self.device)
        return self._tf(imgs)


def image_cache_requested(args, device):
    """train.py --image_cache_gb G > 0 on a HIP device (args built by hand may lack the attribute)."""
    return float(getattr(args, 'image_cache_gb', 0) or 0) > 0 and torch.device(device).type == "cuda"


def image_cache_for(args, dataset, device, max_batch):
    """The DeviceImageCache of a training run over `dataset`, or None: asked for by --image_cache_gb and the
    dataset returns image keys (real COCO; synthetic batches are tensors already)."""
    if not image_cache_requested(args, device) or not getattr(dataset, "return_image_key", False):
        return None
    return DeviceImageCache.from_gb(device, float(args.image_cache_gb), len(dataset.img_ids), max_batch,
                                    present=dataset.present)


def decode_rgb(path):
    """JPEG (any PIL format) -> (H, W, 3) uint8, as the reference's Image.open(...).convert('RGB')
    (dataset.py:55-56)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))
