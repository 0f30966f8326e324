"""Baseline LSTM captioner with the reference surface (models/baseline.py:19-374).

BASELINE.json config 1 ("'baseline' LSTM decoder, batch_size 4 ... on CPU;
plumbing, no GPU"): on CPU tensors the decoder is the plain nn modules (nn.LSTM /
Linear), as in the reference. On HIP tensors forward()
is capmi.baseline_fn.BaselineDecoderFn: the same parameters, hoisted input and
vocabulary GEMMs, the fused LSTM cell per step and a BPTT backward on the capmi
kernels. The ResNet-101 encoder (models.encoder.Encoder) runs the capmi kernels
when given HIP tensors. train() on a HIP device runs capmi.baseline_train.
BaselineTrainStep (one launch per timestep each way, fused CE with ignore_index,
gradients in place, clamp + Adam, HIP graphs, data parallel); forward() and the
autograd path stay as they are. Real COCO on that path goes through the loader of the attention train()
(capmi.imagepipe: packed uint8 images, GPU Resize/ToTensor/Normalize, the device image cache with
--image_cache_gb).
"""
import os
import time

import torch
import torch.nn as nn

from checkpoint import save_checkpoint
from metric import AccumulatingMetric
from models.encoder import Encoder
from train_utils import clip_gradient
from vocabulary import PAD_TOKEN


class BaselineDecoderParams:
    hidden_size = 512
    embed_size = 512  # Use 300 if glove.
    vocab_size = None  # Must override.


class BaselineDecoder(nn.Module):
    def __init__(self, params):
        super().__init__()
        assert isinstance(params, BaselineDecoderParams)
        assert params.vocab_size is not None
        self.embed_size = params.embed_size
        self.hidden_size = params.hidden_size
        self.embedding = nn.Embedding(params.vocab_size, params.embed_size)
        self.lstm = nn.LSTM(input_size=params.embed_size, hidden_size=params.hidden_size, num_layers=1,
                            bias=True, batch_first=True, dropout=0, bidirectional=False)
        self.linear = nn.Linear(params.hidden_size, params.vocab_size)

    def load_pretrained_embeddins(self, embeddings):
        self.embedding.weight = nn.Parameter(embeddings)

    def fine_tune_embeddings(self, on=True):
        for param in self.embedding.parameters():
            param.requires_grad = on

    def _capmi_ws(self, device):
        """stream-K workspace of the decoder's GEMMs (runtime state: not pickled)."""
        ws = self.__dict__.get("_capmi_sk")
        if ws is None or ws.device != torch.device(device):
            from capmi import kernels as K
            ws = K.gemm_workspace(device)
            self.__dict__["_capmi_sk"] = ws
        return ws

    def __getstate__(self):
        st = self.__dict__.copy()
        st.pop("_capmi_sk", None)
        return st

    def forward(self, img_features, captions):
        """(B,M) image features, (B,L) captions -> (B,L,V) scores: the image feature is
        step 0, the caption without <end> follows (reference :81-111)."""
        if img_features.is_cuda:
            from capmi.baseline_fn import baseline_forward
            return baseline_forward(self, img_features, captions)
        captions = captions[:, :-1]
        embeddings = self.embedding(captions)
        embeddings = torch.cat((img_features.unsqueeze(1).float(), embeddings.float()), dim=1)
        lstm_out, _ = self.lstm(embeddings)
        return self.linear(lstm_out)


def train(device, args):
    """Reference :114-264 (CE with ignore_index=PAD against the captions incl. <start>)."""
    from capmi.imagepipe import collate_images
    from models.attention import _train_dataset
    from torch.nn.utils.rnn import pad_sequence
    on_step = torch.device(device).type == "cuda" and os.environ.get("CAPMI_BASELINE_STEP", "1") != "0"
    # on the step, as the attention train(): COCO images stay uint8 and are resized on the GPU, through the device
    # image cache when args.image_cache_gb > 0
    dataset = _train_dataset(args, device if on_step else None)
    pad_idx = dataset.vocab(PAD_TOKEN)

    def collate_fn(data):
        imgs, captions, *keys = zip(*data)
        imgs = collate_images(imgs, *keys) if on_step else torch.stack(imgs, 0)
        return imgs, pad_sequence(captions, batch_first=True, padding_value=pad_idx)

    if on_step:
        return _train_on_step(device, args, dataset, pad_idx, collate_fn)
    # CPU devices, and CAPMI_BASELINE_STEP=0 on the GPU: the reference's autograd loop
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, shuffle=True,
                                         num_workers=args.workers, collate_fn=collate_fn)
    encoder = Encoder(args.embed_size)
    # reference :279-282: only the (trainable) embed Linear, since fine_tune() is never called
    encoder_optimizer = torch.optim.Adam(params=filter(lambda p: p.requires_grad, encoder.parameters()),
                                         lr=args.encoder_lr) if args.fine_tune_encoder else None
    params = BaselineDecoderParams()
    params.embed_size, params.hidden_size, params.vocab_size = args.embed_size, args.decoder_dim, len(dataset.vocab)
    decoder = BaselineDecoder(params)
    if args.use_glove:
        from embed import load_glove_vectors
        decoder.load_pretrained_embeddins(load_glove_vectors())
    decoder.fine_tune_embeddings(on=args.fine_tune_embedding)
    decoder_optimizer = torch.optim.Adam(params=filter(lambda p: p.requires_grad, decoder.parameters()),
                                         lr=args.decoder_lr)
    encoder, decoder = encoder.to(device), decoder.to(device)
    criterion = nn.CrossEntropyLoss(ignore_index=pad_idx).to(device)
    decoder.train()
    encoder.train()
    train_start = time.time()
    num_batches = len(loader)
    epoch_losses = []
    for epoch in range(args.epochs):
        batch_losses = []
        accum_loss, accum_time = AccumulatingMetric(), AccumulatingMetric()
        start = time.time()
        for batch_idx, (imgs, captions) in enumerate(loader):
            imgs, captions = imgs.to(device), captions.to(device)
            scores = decoder(encoder(imgs), captions)
            loss = criterion(scores.reshape(-1, scores.shape[2]), captions.reshape(-1))
            decoder_optimizer.zero_grad()
            if encoder_optimizer is not None:
                encoder_optimizer.zero_grad()
            loss.backward()
            clip_gradient(decoder_optimizer, args.grad_clip)
            if encoder_optimizer is not None:
                clip_gradient(encoder_optimizer, args.grad_clip)
            decoder_optimizer.step()
            if encoder_optimizer is not None:
                encoder_optimizer.step()
            batch_losses.append(loss.item())
            accum_loss.update(loss.item())
            accum_time.update(time.time() - start)
            if batch_idx % args.print_freq == 0:
                print(f'Epoch {epoch+1}/{args.epochs}, Batch {batch_idx+1}/{num_batches}, '
                      f'Loss {accum_loss.avg():.4f}, Time: {accum_time.val:.4f}')
            start = time.time()
        epoch_losses.append(batch_losses)
        save_checkpoint(args, epoch, encoder, decoder, encoder_optimizer, decoder_optimizer,
                        {'epoch_losses': epoch_losses})
    print(f'Model {args.model_name} finished training for {args.epochs} epochs in '
          f'{time.time() - train_start:.4f} seconds.')


def _train_on_step(device, args, dataset, pad_idx, collate_fn):
    """``train`` on a HIP device: the same models, loop and log line on capmi.baseline_train.BaselineTrainStep
    (fused CE with ignore_index, gradients in place, clamp fused into capmi.optim.Adam, one HIP graph per batch
    shape unless CAPMI_TRAIN_GRAPH=0). Losses stay on the device and are read every ``print_freq`` batches and
    at the epoch's end; data-parallel over torchrun ranks when WORLD_SIZE > 1 (rank 0 prints and saves)."""
    from capmi import dist as cdist
    from capmi import kernels as K
    from capmi.baseline_train import BaselineTrainStep
    from capmi.data import synthetic_requested
    from capmi.imagepipe import ImageFeeder, image_cache_for
    from capmi.optim import Adam
    ctx = cdist.init_from_env(device)
    device = ctx.device
    sampler = cdist.sampler_for(dataset, ctx)
    # as in the attention train(): packed COCO pixels are uploaded from pinned memory, and with the image cache
    # the workers live for the whole run
    pin = not synthetic_requested(args)
    keep = args.workers > 0 and getattr(dataset, "return_image_key", False)
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, shuffle=sampler is None,
                                         sampler=sampler, num_workers=args.workers, collate_fn=collate_fn,
                                         pin_memory=pin, persistent_workers=keep)
    feed = ImageFeeder(device, image_cache_for(args, dataset, device, args.batch_size))
    train.last_image_cache = feed.cache  # (tests: its stats)
    encoder = Encoder(args.embed_size)
    params = BaselineDecoderParams()
    params.embed_size, params.hidden_size, params.vocab_size = args.embed_size, args.decoder_dim, len(dataset.vocab)
    decoder = BaselineDecoder(params)
    if args.use_glove:
        from embed import load_glove_vectors
        decoder.load_pretrained_embeddins(load_glove_vectors())
    decoder.fine_tune_embeddings(on=args.fine_tune_embedding)
    encoder, decoder = encoder.to(device), decoder.to(device)
    # every rank starts from rank 0's weights and BN buffers
    cdist.broadcast_module(encoder, ctx)
    cdist.broadcast_module(decoder, ctx)
    # reference :279-282: only the (trainable) embed Linear, since fine_tune() is never called
    encoder_optimizer = Adam(filter(lambda p: p.requires_grad, encoder.parameters()),
                             lr=args.encoder_lr) if args.fine_tune_encoder else None
    decoder_optimizer = Adam(filter(lambda p: p.requires_grad, decoder.parameters()), lr=args.decoder_lr)
    step = BaselineTrainStep(encoder, decoder, decoder_optimizer, ctx,
                             graph=os.environ.get("CAPMI_TRAIN_GRAPH", "1") != "0",
                             encoder_optimizer=encoder_optimizer, ignore_index=pad_idx)
    train.last_step = step  # (tests: which launch mode ran)
    if pin and args.workers > 0:  # the loader's pin-memory thread allocates while a step is being captured
        step.capture_error_mode = "thread_local"
    decoder.train()
    encoder.train()
    train_start = time.time()
    num_batches = len(loader)
    epoch_losses = []
    for epoch in range(args.epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        batch_losses, pending = [], []
        accum_loss, accum_time = AccumulatingMetric(), AccumulatingMetric()
        start = time.time()
        for batch_idx, (imgs, captions) in enumerate(loader):
            imgs, captions = feed(imgs), captions.to(device, non_blocking=True)
            clip_gradient(decoder_optimizer, args.grad_clip)
            if encoder_optimizer is not None:
                clip_gradient(encoder_optimizer, args.grad_clip)
            pending.append(step(imgs, captions).detach().clone())  # the step's own buffer: the next call reuses it
            if batch_idx % args.print_freq == 0 or batch_idx == num_batches - 1:
                torch.cuda.synchronize()
                K.sk_check()  # stream-K hand-off invariant (raises on a timed-out hand-off)
                for l in torch.stack(pending).view(-1).tolist():
                    batch_losses.append(l)
                    accum_loss.update(l)
                pending = []
                accum_time.update(time.time() - start)
                if ctx.rank == 0 and batch_idx % args.print_freq == 0:
                    print(f'Epoch {epoch+1}/{args.epochs}, Batch {batch_idx+1}/{num_batches}, '
                          f'Loss {accum_loss.avg():.4f}, Time: {accum_time.val:.4f}')
            start = time.time()
        epoch_losses.append(batch_losses)
        if ctx.rank == 0:
            save_checkpoint(args, epoch, encoder, decoder, encoder_optimizer, decoder_optimizer,
                            {'epoch_losses': epoch_losses})
    if ctx.rank == 0:
        print(f'Model {args.model_name} finished training for {args.epochs} epochs in '
              f'{time.time() - train_start:.4f} seconds.')


class _KeyedItems(torch.utils.data.Dataset):
    """(image, caption, key) items of a dataset whose items are (image, caption): the key is the item's index
    (SyntheticCOCO: one image per item)."""

    def __init__(self, dataset):
        self.dataset, self.vocab = dataset, dataset.vocab

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, i):
        img, cap = self.dataset[i][:2]
        return img, cap, i


def check_self_critical_args(args):
    """What ``--self_critical True`` asks of the other flags, before any data is loaded."""
    if args.model != 'baseline':
        raise NotImplementedError('--self_critical True: only --model baseline has a self-critical step '
                                  '(the attention captioner needs its features repeated per sample)')
    if not getattr(args, 'checkpoint', None):
        raise SystemExit('--self_critical True continues from a cross-entropy trained model: give --checkpoint '
                         '(a baseline state-dict checkpoint in ./checkpoints)')
    if args.fine_tune_encoder:
        raise NotImplementedError('--self_critical True with --fine_tune_encoder True: the features are computed '
                                  'once per step, without a graph')
    if not 0 <= args.sc_max_len <= 63:
        raise SystemExit('--sc_max_len must be 0..63 (a sampled caption holds at most 64 words)')


def train_self_critical(device, args):
    """Self-critical training of a cross-entropy trained baseline captioner (capmi.scst): ``--checkpoint`` is
    loaded as eval.py --model_type baseline loads it (sizes read off the tensors), the CIDEr-D tables are built
    from the training set's captions grouped by image, and the loop of ``_train_on_step`` runs on
    BaselineSelfCriticalStep over the distinct images of every batch. Loss, reward and (``--sc_baseline greedy``)
    the greedy reward stay on the device and are read every ``print_freq`` batches and at the epoch's end."""
    from capmi import dist as cdist
    from capmi.scst import BaselineSelfCriticalStep
    from checkpoint import load_checkpoint, unpack_checkpoint
    check_self_critical_args(args)
    ctx, device, base, dataset, refs = self_critical_data(device, args)
    _, enc_sd, dec_sd, _, _, _ = unpack_checkpoint(
        load_checkpoint(device, args, verbose=ctx.rank == 0, weights_only=not getattr(args, "trusted_checkpoint", False)))
    if hasattr(dec_sd, 'state_dict'):  # a whole-module checkpoint
        enc_sd, dec_sd = enc_sd.state_dict(), dec_sd.state_dict()
    if len(dataset.vocab) != dec_sd["linear.weight"].shape[0]:
        raise SystemError(f'checkpoint decodes {dec_sd["linear.weight"].shape[0]} words, the vocabulary has '
                          f'{len(dataset.vocab)}')
    encoder = Encoder(enc_sd["embed.weight"].shape[0])
    encoder.load_state_dict(enc_sd)
    params = BaselineDecoderParams()
    params.embed_size, params.hidden_size = dec_sd["embedding.weight"].shape[1], dec_sd["lstm.weight_hh_l0"].shape[1]
    params.vocab_size = dec_sd["linear.weight"].shape[0]
    decoder = BaselineDecoder(params)
    if dec_sd["embedding.weight"].dtype == torch.float64:  # GloVe tables stay fp64
        decoder.load_pretrained_embeddins(dec_sd["embedding.weight"].clone())
    decoder.load_state_dict(dec_sd)
    encoder, decoder = encoder.to(device), decoder.to(device)
    cdist.broadcast_module(encoder, ctx)
    cdist.broadcast_module(decoder, ctx)
    self_critical_loop(args, ctx, device, base, dataset, refs, encoder, decoder, BaselineSelfCriticalStep,
                       train_self_critical)


def self_critical_data(device, args):
    """The data side of self-critical training, for either captioner: (ctx, device, the training set, its (image,
    caption, key) items, the ``CiderRefs`` of its captions grouped by image, END appended; with
    ``args.sc_reward_mix`` set, the ``capmi.devscore.ScoreRefs`` of the same captions)."""
    from capmi import dist as cdist
    from capmi.data import synthetic_requested
    from capmi.scst import MAX_REF_WORDS, CiderRefs
    from vocabulary import END_TOKEN, START_TOKEN
    if torch.device(device).type != "cuda":
        raise RuntimeError("self-critical training runs on a HIP device (the rollouts and the reward are kernels)")
    ctx = cdist.init_from_env(device)
    device = ctx.device
    if synthetic_requested(args):
        from capmi.data import SyntheticCOCO
        base = SyntheticCOCO.from_args(args)
        dataset, n_images = _KeyedItems(base), len(base)
    else:
        from dataset import COCODataset  # real COCO path (needs pycocotools or capmi.coco, images)
        dataset = base = COCODataset(mode='train', caption_max_len=args.max_caption_length, return_image_key=True)
        n_images = len(base.img_ids)
    vocab = dataset.vocab
    end_idx = vocab(END_TOKEN)
    special = {vocab(PAD_TOKEN), vocab(START_TOKEN), end_idx}
    tables = CiderRefs
    if getattr(args, "sc_reward_mix", None) is not None:  # a mixed reward reads the BLEU / ROUGE-L tables too
        from capmi.devscore import ScoreRefs as tables
    refs = tables.build([[[w for w in cap.tolist() if w not in special][:MAX_REF_WORDS] for cap in base.references(k)]
                         for k in range(n_images)], end_idx=end_idx, device=device)
    return ctx, device, base, dataset, refs


def self_critical_loop(args, ctx, device, base, dataset, refs, encoder, decoder, step_class, owner):
    """The training loop of self-critical training on ``step_class`` (capmi.scst) over the distinct images of
    every batch; ``owner.last_step`` keeps the step (tests: which launch mode ran)."""
    from capmi import dist as cdist
    from capmi import kernels as K
    from capmi.data import synthetic_requested
    from capmi.imagepipe import ImageFeeder, collate_images, image_cache_for
    from capmi.optim import Adam
    from vocabulary import END_TOKEN, START_TOKEN
    vocab = dataset.vocab
    pad_idx, start_idx, end_idx = vocab(PAD_TOKEN), vocab(START_TOKEN), vocab(END_TOKEN)
    decoder.fine_tune_embeddings(on=args.fine_tune_embedding)
    for q in encoder.parameters():  # the features are inputs here
        q.requires_grad = False
    encoder.eval()
    decoder.train()
    cache = image_cache_for(args, base, device, args.batch_size)

    def collate_fn(data):
        seen, keep = set(), []
        for item in data:  # an image appears once per step
            if item[2] not in seen:
                seen.add(item[2])
                keep.append(item)
        imgs, _, keys = zip(*keep)
        return collate_images(imgs, keys if cache is not None else None), torch.tensor(keys, dtype=torch.int32)

    sampler = cdist.sampler_for(dataset, ctx)
    pin = not synthetic_requested(args)
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, shuffle=sampler is None,
                                         sampler=sampler, num_workers=args.workers, collate_fn=collate_fn,
                                         pin_memory=pin, persistent_workers=args.workers > 0 and cache is not None)
    feed = ImageFeeder(device, cache)
    decoder_optimizer = Adam(filter(lambda p: p.requires_grad, decoder.parameters()), lr=args.decoder_lr)
    mix = getattr(args, "sc_reward_mix", None)  # weights of CIDEr-D, BLEU-4, ROUGE-L (capmi.scst); no train.py flag
    step = step_class(encoder, decoder, decoder_optimizer, refs, ctx, num_samples=args.sc_samples,
                      temperature=args.sc_temperature, top_k=args.sc_top_k, baseline=args.sc_baseline,
                      max_steps=args.sc_max_len, score_end=True, graph=os.environ.get("CAPMI_TRAIN_GRAPH", "1") != "0",
                      start_idx=start_idx, end_idx=end_idx, pad_idx=pad_idx, reward_mix=mix)
    owner.last_step = step
    if pin and args.workers > 0:  # the loader's pin-memory thread allocates while a step is being captured
        step.capture_error_mode = "thread_local"
    greedy = args.sc_baseline == "greedy"
    seed0 = int(torch.initial_seed()) % (1 << 31) + 7919 * ctx.rank
    train_start = time.time()
    num_batches = len(loader)
    epoch_losses, epoch_rewards, it = [], [], 0
    for epoch in range(args.epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        batch_losses, batch_rewards, pending = [], [], []
        accum = [AccumulatingMetric() for _ in range(3 if mix is None else 6)]
        accum_time = AccumulatingMetric()
        start = time.time()
        for batch_idx, (imgs, keys) in enumerate(loader):
            clip_gradient(decoder_optimizer, args.grad_clip)
            loss = step(feed(imgs), keys, seed=seed0 + it)
            it += 1
            # the step's own buffers: the next call reuses them
            pending.append(torch.cat([loss.detach(), step.last["reward_mean"],
                                      step.last["greedy_reward_mean"] if greedy else loss.detach()]
                                     + ([step.last[k].mean().reshape(1) for k in ("cider", "bleu4", "rouge_l")]
                                        if mix is not None else [])))
            if batch_idx % args.print_freq == 0 or batch_idx == num_batches - 1:
                torch.cuda.synchronize()
                K.sk_check()
                for l, r, g, *parts in torch.stack(pending).tolist():
                    batch_losses.append(l)
                    batch_rewards.append(r)
                    for a, v in zip(accum, (l, r, g, *parts)):
                        a.update(v)
                pending = []
                accum_time.update(time.time() - start)
                if ctx.rank == 0 and batch_idx % args.print_freq == 0:
                    print(f'Epoch {epoch+1}/{args.epochs}, Batch {batch_idx+1}/{num_batches}, '
                          f'Loss {accum[0].avg():.4f}, Reward {accum[1].avg():.4f}, '
                          + (f'Greedy {accum[2].avg():.4f}, ' if greedy else '')
                          + (f'CIDEr-D {accum[3].avg():.4f}, BLEU-4 {accum[4].avg():.4f}, '
                             f'ROUGE-L {accum[5].avg():.4f}, ' if mix is not None else '')
                          + f'Time: {accum_time.val:.4f}')
            start = time.time()
        epoch_losses.append(batch_losses)
        epoch_rewards.append(batch_rewards)
        if ctx.rank == 0:
            save_checkpoint(args, epoch, encoder, decoder, None, decoder_optimizer,
                            {'epoch_losses': epoch_losses, 'epoch_rewards': epoch_rewards})
    if ctx.rank == 0:
        print(f'Model {args.model_name} finished self-critical training for {args.epochs} epochs in '
              f'{time.time() - train_start:.4f} seconds.')


def _eval_dataset(args):
    """``args.dataset`` when the caller supplies one (items ``(img, caption)``, a ``vocab``), synthetic ragged
    captions for ``synthetic_size > 0``, else the reference's COCO 'val' set (needs the dataset)."""
    dataset = getattr(args, "dataset", None)
    if dataset is not None:
        return dataset
    n = int(getattr(args, "synthetic_size", 0) or 0)
    if n > 0:
        from capmi.data import SyntheticCOCO
        return SyntheticCOCO(n, V=int(getattr(args, "vocab_size", 8100)), L=int(getattr(args, "synthetic_len", 25)),
                             ragged=True)
    from dataset import COCODataset  # real COCO path (pycocotools, nltk, images)
    return COCODataset(mode='val', caption_max_len=getattr(args, "max_caption_length", -1))


def _eval_loader(args, dataset, batch_size):
    from torch.nn.utils.rnn import pad_sequence
    pad_idx = dataset.vocab(PAD_TOKEN)

    def collate_fn(data):
        imgs, captions = list(zip(*data))[:2]
        return (torch.stack(imgs, dim=0), pad_sequence(captions, batch_first=True, padding_value=pad_idx),
                [len(c) for c in captions])  # true lengths

    return torch.utils.data.DataLoader(dataset=dataset, batch_size=int(batch_size), shuffle=False,
                                       num_workers=int(getattr(args, "workers", 0) or 0), collate_fn=collate_fn)


def evaluate(device, args, encoder, decoder):
    """Reference :267-374: one teacher-forced pass over the validation set at batch 1. Step 0 is fed the image
    feature and scored against START, step t the embedding of caption[t-1] against caption[t]; loss = the plain
    CE mean over the caption's n rows; hypotheses = the greedy tokens, references = the caption repeated n
    times, both with START / END / PAD removed.

    ``args.batch_size`` (default 1) above 1 runs ``evaluate_batched``, whose per-caption numbers are the same.
    The loop goes through ``decoder.forward``: plain nn.LSTM on CPU tensors, capmi.baseline_fn on HIP tensors.
    Caption scoring (metric.get_eval_score) is attempted and skipped when unavailable: the returned dict then
    holds the losses, references and hypotheses."""
    from metric import get_eval_score
    from vocabulary import END_TOKEN, START_TOKEN
    batch_size = int(getattr(args, "batch_size", 1) or 1)
    if batch_size > 1:
        return evaluate_batched(device, args, encoder, decoder, batch_size=batch_size)
    dataset = _eval_dataset(args)
    vocab = dataset.vocab
    drop = {vocab(START_TOKEN), vocab(END_TOKEN), vocab(PAD_TOKEN)}
    loader = _eval_loader(args, dataset, 1)
    print_freq = int(getattr(args, "print_freq", 1) or 1)
    references, hypotheses, losses = [], [], []
    accum_loss = AccumulatingMetric()
    decoder.eval()
    encoder.eval()
    num_batches = len(loader)
    start_time = time.time()
    with torch.no_grad():
        for batch_idx, (imgs, captions, _) in enumerate(loader):
            imgs, captions = imgs.to(device), captions.to(device)
            scores = decoder(encoder(imgs), captions)  # (1, n, V)
            loss = nn.functional.cross_entropy(scores.reshape(-1, scores.shape[2]), captions.reshape(-1))
            n = captions.shape[1]
            accum_loss.update(loss.item(), n)
            losses.append(loss.item())
            for cap in captions.tolist():
                ref = [w for w in cap if w not in drop]
                references.append([ref for _ in cap])  # reference :345-350
            preds = torch.max(scores, dim=2)[1].tolist()
            hypotheses.extend([[w for w in p if w not in drop] for p in preds])
            if batch_idx % print_freq == 0:
                print(f'Batch {batch_idx+1}/{num_batches}, Loss {accum_loss.avg():.4f}')
    try:
        metrics = get_eval_score(references, hypotheses)
    except (NotImplementedError, ImportError):
        metrics = {"references": references, "hypotheses": hypotheses}
    metrics['losses'] = losses
    print(f'Checkpoint {getattr(args, "checkpoint", None)} finished evaluation in '
          f'{time.time() - start_time:.4f} seconds.')
    return metrics


def evaluate_batched(device, args, encoder, decoder, dataset=None, batch_size=64):
    """The validation pass of ``evaluate`` over ``batch_size`` captions per step, with per-caption results
    equal to what the reference computes one caption at a time (reference :267-374 at batch 1).

    Captions are taken in dataset order (no shuffle), padded to the batch maximum and passed with their true
    lengths. Per batch: one encoder forward, capmi.baseline_eval.BaselineTeacherForcedEval (loss, greedy tokens
    and top-1 / top-5 counts on the device), one asynchronous copy of the small result buffer to pinned host
    memory; the device is synchronised only every ``print_freq`` batches and at the end. The vocabulary is the
    dataset's (the baseline decoder has none).

    Returns a JSON-serialisable dict: the capmi.scoring.caption_scores keys, ``losses`` (per caption, dataset
    order), ``loss`` (their average weighted by caption length n), ``top1_acc`` / ``top5_acc`` over all scored
    rows, ``references`` and ``hypotheses`` (as ``evaluate`` builds them)."""
    from capmi import baseline_eval
    from capmi.scoring import caption_scores
    from vocabulary import END_TOKEN, START_TOKEN
    if dataset is None:
        dataset = _eval_dataset(args)
    vocab = dataset.vocab
    drop = {vocab(START_TOKEN), vocab(END_TOKEN), vocab(PAD_TOKEN)}
    loader = _eval_loader(args, dataset, batch_size)
    print_freq = int(getattr(args, "print_freq", 1) or 1)
    on_gpu = torch.device(device).type == "cuda"
    tf_eval = baseline_eval.BaselineTeacherForcedEval(decoder)
    evaluate_batched.last_eval = tf_eval  # (tests: its last_stats)
    references, hypotheses, losses = [], [], []
    hits1 = hits5 = rows = 0
    accum_loss = AccumulatingMetric()
    decoder.eval()
    encoder.eval()
    num_batches = len(loader)
    start_time = time.time()
    pending = []

    def drain():
        nonlocal hits1, hits5, rows
        if on_gpu:
            torch.cuda.synchronize()
        for host, caps_h, lengths, T in pending:
            res = baseline_eval.unpack(host, len(lengths), T)
            loss_h, pred_h = res["cap_loss"].tolist(), res["pred"].tolist()
            hits1 += int(res["top1"].sum())
            hits5 += int(res["top5"].sum())
            for i, n in enumerate(lengths):
                accum_loss.update(loss_h[i], n)
                losses.append(loss_h[i])
                rows += n
                ref = [w for w in caps_h[i][:n] if w not in drop]
                references.append([ref for _ in range(n)])  # reference :345-350, at this caption's own length
                hypotheses.append([w for w in pred_h[i][:n] if w not in drop])
        del pending[:]

    with torch.no_grad():
        for batch_idx, (imgs, captions, caption_lengths) in enumerate(loader):
            imgs = imgs.to(device, non_blocking=True)
            res = tf_eval(encoder(imgs), captions.to(device, non_blocking=True), caption_lengths)
            packed = res["packed"]
            host = torch.empty(packed.shape, dtype=packed.dtype, pin_memory=on_gpu)
            host.copy_(packed, non_blocking=True)
            pending.append((host, captions.tolist(), caption_lengths, res["pred"].shape[1]))
            if batch_idx % print_freq == 0:
                drain()
                print(f'Batch {batch_idx+1}/{num_batches}, Loss {accum_loss.avg():.4f}')
        drain()
    if getattr(args, "scorer", "host") == "device":  # the counting on the device (capmi.devscore)
        from capmi.devscore import caption_scores_device
        metrics = caption_scores_device(references, hypotheses, device)
    else:
        metrics = caption_scores(references, hypotheses)
    metrics.update(losses=losses, loss=accum_loss.avg(), top1_acc=hits1 / max(rows, 1), top5_acc=hits5 / max(rows, 1),
                   references=references, hypotheses=hypotheses)
    print(f'Checkpoint {getattr(args, "checkpoint", None)} finished evaluation in '
          f'{time.time() - start_time:.4f} seconds.')
    return metrics


def evaluate_generated(device, args, encoder, decoder, dataset=None, batch_size=64):
    """Validation on generated captions (capmi.genval), as models.attention.evaluate_generated: every image of
    ``dataset`` (default: ``_eval_dataset(args)``) captioned once by ``BaselineBatchedBeamSearch`` and scored against
    all of its references on the device. The vocabulary is the dataset's. Same arguments read off ``args``
    (``beam_size``, ``max_decode_len``, ``length_alpha``, ``print_freq``), same returned keys."""
    from capmi import genval
    from capmi.beam import BaselineBatchedBeamSearch
    if torch.device(device).type != "cuda":
        raise RuntimeError("generated-caption validation runs on a HIP device (the search and the scores are kernels)")
    if dataset is None:
        dataset = _eval_dataset(args)
    search = BaselineBatchedBeamSearch(decoder, int(getattr(args, "beam_size", 3)))
    return genval.evaluate_generated(device, args, encoder, decoder, search, dataset, dataset.vocab, batch_size)
