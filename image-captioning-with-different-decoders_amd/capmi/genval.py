"""Validation on generated captions: every image captioned once with beam search and scored against all of its
references, with the captions and the counting on the device.

``PerImageView``           one item per image of a caption dataset, ``(img, key)`` in ``img_ids`` order, and the image's
                           ``references(key)``
``build_refs``             the ``capmi.devscore.ScoreRefs`` of a view's references (START / END / PAD stripped, cut to the
                           scorer's limit, no END appended: the tables ``caption_scores_device`` builds)
``GeneratedCaptionEval``   per batch: encoder forward, ``search_device`` (beam search with the back-trace on the device,
                           capmi_beam_backtrack), ``DeviceCaptionScorer.score_table`` on the token table it leaves, and
                           device-to-device copies of the rows into tables of the whole set; ``results`` brings them to
                           the host once
``evaluate_generated``     the pass over a dataset that models.attention / models.baseline call with their search

The teacher-forced passes (``evaluate`` / ``evaluate_batched``) score the argmax under the ground-truth prefix, once
per caption against that caption; this pass scores what the captioner writes on its own, which is what self-critical
training changes.
"""
import time

import torch

from ._lib import CAPMI_SCORE_STATS
from .devscore import DeviceCaptionScorer, ScoreRefs, _cider_listing, corpus_scores_from_rows
from .scst import MAX_HYP_WORDS, MAX_REF_WORDS, MAX_TOKEN


class PerImageView(torch.utils.data.Dataset):
    """Items ``(img, key)``, one per image: a ``COCODataset`` is viewed by its ``img_ids`` (key = the index in
    them), any other dataset by its items (``SyntheticCOCO``: one image per item, key = the item's index)."""

    def __init__(self, dataset):
        self.dataset, self.vocab = dataset, dataset.vocab
        self.by_img_ids = hasattr(dataset, "img_ids")
        self.keys = list(range(len(dataset.img_ids) if self.by_img_ids else len(dataset)))

    def __len__(self):
        return len(self.keys)

    def __getitem__(self, i):
        key = self.keys[i]
        if self.by_img_ids:
            return self.dataset._get_transformed_img(self.dataset.img_ids[key]), key
        return self.dataset[key][0], key

    def references(self, key):
        return self.dataset.references(key)


def build_refs(view, special, device):
    """(the ``ScoreRefs`` of every image of ``view`` on ``device``, the references per image): every caption of an
    image without the ``special`` tokens, cut to ``MAX_REF_WORDS``, listed as ``caption_scores_device`` lists
    them. CIDEr's document frequencies are those of the evaluated set."""
    references = [[[int(w) for w in cap.tolist() if int(w) not in special][:MAX_REF_WORDS]
                   for cap in view.references(key)] for key in view.keys]
    listed = [_cider_listing([tuple(r) for r in refs]) for refs in references]
    return ScoreRefs.build(listed, device=device), references


class GeneratedCaptionEval:
    """Captions and scores the images of a set batch by batch. ``search``: a ``BatchedBeamSearch`` or
    ``BaselineBatchedBeamSearch`` of ``decoder``; ``refs``: the ``ScoreRefs`` of the set's ``n_images`` on the HIP
    device, built without ``end_idx``; image ``key`` is row ``key`` of every table."""

    def __init__(self, encoder, decoder, search, refs, start_idx=None, end_idx=None, pad_idx=None, max_decode_len=50,
                 length_alpha=0.0, sync_every=8):
        if not 0 <= int(max_decode_len) <= MAX_HYP_WORDS - 1:
            raise ValueError(f"max_decode_len must be 0..{MAX_HYP_WORDS - 1} (the scorer takes a hypothesis of at "
                             f"most {MAX_HYP_WORDS} words)")
        if not isinstance(refs, ScoreRefs) or refs.end_idx is not None:
            raise ValueError("GeneratedCaptionEval needs a ScoreRefs built without end_idx")
        self.encoder, self.decoder, self.search, self.refs = encoder, decoder, search, refs
        self.start_idx, self.end_idx, self.pad_idx = int(start_idx), int(end_idx), int(pad_idx)
        self.max_decode_len, self.length_alpha, self.sync_every = int(max_decode_len), float(length_alpha), sync_every
        self.scorer = DeviceCaptionScorer(refs)
        N, T, dev = refs.n_images, self.max_decode_len + 1, refs.device
        i32 = dict(dtype=torch.int32, device=dev)
        self.keys = torch.arange(N, **i32)
        self.stats = torch.zeros(N, CAPMI_SCORE_STATS, **i32)
        self.cider = torch.zeros(N, dtype=torch.float32, device=dev)
        self.tokens = torch.full((T, N), -1, **i32)
        self.lens, self.finished = torch.zeros(N, **i32), torch.zeros(N, **i32)
        self.host_syncs = 0  # the search's sync_every reads, over all batches

    @torch.no_grad()
    def step(self, imgs, keys):
        """One batch: ``imgs`` on the device, ``keys`` their image keys on the host, consecutive (the rows of the
        tables the batch fills are one slice). Nothing comes to the host but the search's ``sync_every`` reads."""
        keys = [int(k) for k in keys]
        if keys != list(range(keys[0], keys[0] + len(keys))) or not 0 <= keys[0] <= self.refs.n_images - len(keys):
            raise ValueError("a batch takes consecutive image keys of the tables (a loader in key order, unshuffled)")
        feats = self.encoder(imgs)
        if feats.size(0) != len(keys):
            raise ValueError("one image key per image")
        rows = slice(keys[0], keys[0] + len(keys))
        out = self.search.search_device(feats, self.start_idx, self.end_idx, max_steps=self.max_decode_len,
                                        sync_every=self.sync_every, emit_end=False,
                                        drop=(self.start_idx, self.pad_idx), fallback_live=True,
                                        length_alpha=self.length_alpha)
        sc = self.scorer.score_table(out["tokens"], out["lens"], self.keys[rows])
        self.stats[rows].copy_(sc["stats"])
        self.cider[rows].copy_(sc["cider"])
        self.tokens[:, rows].copy_(out["tokens"])
        self.lens[rows].copy_(out["lens"])
        self.finished[rows].copy_(out["finished"])
        self.host_syncs += self.search.last_stats["host_syncs"]

    def results(self):
        """The tables to the host, once: the six corpus scores, ``hypotheses`` (token ids per image, in key order),
        ``unfinished`` (images that took the live fallback or came out empty), ``mean_length`` and ``host_syncs``
        (the searches' ``sync_every`` reads over all batches)."""
        lens = self.lens.cpu().tolist()
        cols = self.tokens.t().cpu().tolist()
        out = corpus_scores_from_rows(self.stats.cpu().numpy(), self.cider.cpu().numpy())
        out["hypotheses"] = [col[:n] for col, n in zip(cols, lens)]
        out["unfinished"] = int(len(lens) - int(self.finished.sum().item()))
        out["mean_length"] = float(sum(lens) / len(lens))
        out["host_syncs"] = self.host_syncs
        return out


def evaluate_generated(device, args, encoder, decoder, search, dataset, vocab, batch_size=64):
    """The pass of ``models.attention.evaluate_generated`` / ``models.baseline.evaluate_generated`` (which check the
    device) with their ``search`` over ``dataset`` (a caption dataset; viewed per image here). ``captions_per_s``
    counts everything from the reference tables' build to the scores."""
    from vocabulary import END_TOKEN, PAD_TOKEN, START_TOKEN
    from .imagepipe import ImageFeeder, collate_images
    if len(vocab) > MAX_TOKEN + 1:
        raise ValueError(f"the vocabulary must not exceed {MAX_TOKEN + 1} words (16-bit n-gram fields)")
    start_idx, end_idx, pad_idx = vocab(START_TOKEN), vocab(END_TOKEN), vocab(PAD_TOKEN)
    view = dataset if isinstance(dataset, PerImageView) else PerImageView(dataset)
    torch.cuda.synchronize()
    start_time = time.time()
    refs, _ = build_refs(view, {start_idx, end_idx, pad_idx}, device)
    ev = GeneratedCaptionEval(encoder, decoder, search, refs, start_idx, end_idx, pad_idx,
                              max_decode_len=int(getattr(args, "max_decode_len", 50)),
                              length_alpha=float(getattr(args, "length_alpha", 0.0)))

    def collate_fn(data):
        imgs, keys = zip(*data)
        return collate_images(imgs), keys

    # in key order: ``step`` takes a batch of consecutive keys (it refuses any other)
    loader = torch.utils.data.DataLoader(dataset=view, batch_size=int(batch_size), shuffle=False,
                                         num_workers=int(getattr(args, "workers", 0) or 0), collate_fn=collate_fn)
    feed = ImageFeeder(device)
    print_freq = int(getattr(args, "print_freq", 1) or 1)
    decoder.eval()
    encoder.eval()
    num_batches, done = len(loader), 0
    for batch_idx, (imgs, keys) in enumerate(loader):
        imgs = feed(imgs)
        ev.step(imgs, keys)
        done += imgs.size(0)
        if batch_idx % print_freq == 0:
            torch.cuda.synchronize()
            print(f'Batch {batch_idx+1}/{num_batches}, {done / (time.time() - start_time):.1f} captions/s')
    metrics = ev.results()
    elapsed = time.time() - start_time
    metrics.update(image_keys=list(view.keys), captions_per_s=len(view) / elapsed)
    print(f'Checkpoint {getattr(args, "checkpoint", None)} finished generated-caption evaluation in '
          f'{elapsed:.4f} seconds.')
    return metrics
