"""Soft-attention captioning decoder with the reference surface
(models/attention.py of SarahAlkhateeb/Image-Captioning-with-Different-Decoders).

Same classes, constructor arguments, sub-module attributes and state-dict keys
(``attention.{enc_att,dec_att,full_att}``, ``decode_step``, ``h_lin``, ``c_lin``,
``f_beta``, ``fc``, ``embedding``), same forward signatures and outputs. The
compute runs on libcapmi's HIP kernels (capmi.decoder_core): forward,
backward-through-time, fused CE + regulariser and the clamp+Adam update.
"""
import os
import time

import torch
import torch.nn as nn

from capmi import decoder_fn as DF
from capmi import kernels as K
from capmi.optim import Adam as FusedAdam
from checkpoint import load_checkpoint, save_checkpoint, unpack_checkpoint
from metric import AccumulatingMetric
from models.encoder import EncoderAttention
from train_utils import clip_gradient
from vocabulary import PAD_TOKEN, Vocabulary


class SoftAttention(nn.Module):
    """Attention network (reference :18-61). ReLU score (the reference's, not tanh)."""

    def __init__(self, encoder_dim=2048, decoder_dim=512, attention_dim=512):
        super(SoftAttention, self).__init__()
        self.enc_att = nn.Linear(encoder_dim, attention_dim)
        self.dec_att = nn.Linear(decoder_dim, attention_dim)
        self.full_att = nn.Linear(attention_dim, 1)
        self.relu = nn.ReLU()
        self.softmax = nn.Softmax(dim=1)

    def forward(self, encoder_out, decoder_hidden):
        """(B,P,E), (B,D) -> attention-weighted encoding (B,E), weights (B,P)."""
        return DF.soft_attention_forward(self, encoder_out, decoder_hidden)


class AttentionDecoderParams:
    attention_dim = 512
    decoder_dim = 512
    embed_size = 512  # Use 300 if glove and 768 if BERT.
    dropout = 0.5
    use_bert = False
    vocab = None  # Must override.


class AttentionDecoder(nn.Module):
    """Reference :72-284."""

    def __init__(self, device, params):
        super(AttentionDecoder, self).__init__()
        assert isinstance(params, AttentionDecoderParams)
        assert isinstance(params.vocab, Vocabulary)
        self.device = device
        self.encoder_dim = 2048  # Set in stone.
        self.attention_dim = params.attention_dim
        self.embed_size = params.embed_size
        self.decoder_dim = params.decoder_dim
        self.vocab = params.vocab
        self.vocab_size = len(self.vocab)
        self.dropout = params.dropout
        self.use_bert = params.use_bert
        # reference :96-100 loads bert-base-uncased by name (a network fetch, unavailable offline).
        # The BERT variant is kept as its interface: ``bert_embedder(encoded_captions)`` returns
        # the (B, L+1, 768) word-level layer-11 features that _create_bert_embeddings (:166-215)
        # builds: capmi.bert.BertEmbedder over a local checkpoint (train.py --bert_path; the real BERT
        # forward on the HIP kernels), or capmi.data.SyntheticBertEmbedder for benchmarks. A plain
        # attribute, not a submodule: state-dict keys and checkpoints are the same with and without it.
        self.bert_embedder = None
        self.compute_precision = "fp32"  # set_compute_precision

        self.attention = SoftAttention(self.encoder_dim, self.decoder_dim, self.attention_dim)
        self.dropout = nn.Dropout(p=self.dropout)
        self.decode_step = nn.LSTMCell(self.embed_size + self.encoder_dim, self.decoder_dim, bias=True)
        self.h_lin = nn.Linear(self.encoder_dim, self.decoder_dim)
        self.c_lin = nn.Linear(self.encoder_dim, self.decoder_dim)
        self.f_beta = nn.Linear(self.decoder_dim, self.encoder_dim)
        self.sigmoid = nn.Sigmoid()
        self.fc = nn.Linear(self.decoder_dim, self.vocab_size)
        self.embedding = nn.Embedding(self.vocab_size, self.embed_size)

        # reference :119-126
        self.fc.bias.data.fill_(0)
        self.fc.weight.data.uniform_(-0.1, 0.1)
        self.embedding.weight.data.uniform_(-0.1, 0.1)
        self.fine_tune_embeddings(on=True)

    def set_compute_precision(self, precision):
        """Arithmetic of the decoder's GEMMs on the MI355X (the per-step attention / LSTMCell
        pointwise, softmax and loss kernels stay fp32 throughout): 'fp32' (the reference's, fp32
        MFMA), 'fp32-x3' (fp32-accurate: both operands split exactly into three bf16 terms on the
        bf16 matrix cores, as the encoder's 'fp32-x3') or 'bf16' (operands rounded to bf16, fp32
        accumulation: the bf16 config, BASELINE config 5)."""
        if precision not in ("fp32", "fp32-x3", "bf16"):
            raise ValueError(precision)
        self.compute_precision = precision

    def load_pretrained_embeddins(self, embeddings):
        """Reference :128-136 (name kept, typo included). GloVe tables stay fp64 (Q7)."""
        self.embedding.weight = nn.Parameter(embeddings)

    def fine_tune_embeddings(self, on=True):
        for param in self.embedding.parameters():
            param.requires_grad = on

    def bert_embeddings(self, encoded_captions):
        """Reference _create_bert_embeddings (:166-215): (B, L) tokens -> (B, L+1, 768) features."""
        if self.bert_embedder is None:
            raise RuntimeError("use_bert=True needs decoder.bert_embedder (bert-base-uncased cannot be "
                               "fetched offline; see capmi.data.SyntheticBertEmbedder)")
        return self.bert_embedder(encoded_captions)

    def init_hidden_state(self, encoder_out):
        """(B,P,E) -> h, c (B,D) (reference :151-164)."""
        return DF.init_hidden_forward(self, encoder_out)

    def forward(self, encoder_out, encoded_captions, caption_lengths):
        """(B,14,14,E), (B,L) int64, list[int] -> predictions (B,T,V), captions,
        decode_lengths, alphas (B,T,P)   (reference :218-284)."""
        return DF.decoder_forward(self, encoder_out, encoded_captions, caption_lengths)


# ======================================================================================
# training (reference :287-452)
# ======================================================================================
def _train_dataset(args, device=None):
    """The training set of train() (here and in models.baseline): synthetic, or COCO without a transform
    (decoded uint8 images, resized on the GPU), with image keys when --image_cache_gb asks for the device
    image cache on a HIP `device`."""
    from capmi.data import SyntheticCOCO, synthetic_requested
    if synthetic_requested(args):
        return SyntheticCOCO.from_args(args)
    from capmi.imagepipe import image_cache_requested
    from dataset import COCODataset  # real COCO path (needs pycocotools, nltk, images)
    return COCODataset(mode='train', caption_max_len=args.max_caption_length,
                       return_image_key=device is not None and image_cache_requested(args, device))


def _build_models(args, vocab, device):
    """Encoder + decoder of train() (reference :329-364): fresh from the args, or resumed from
    ``args.checkpoint`` (state_dict or whole-module format). Returns (encoder, decoder,
    start_epoch, metrics, decoder optimizer state, encoder optimizer state)."""
    enc_opt_state = None
    if args.checkpoint is None:
        encoder = EncoderAttention()
        if args.fine_tune_encoder:
            # the reference builds Adam over an all-frozen encoder here and crashes (Q9);
            # fine-tuning means fine_tune(True): layer2-4 trainable (models/encoder.py:112-121)
            encoder.fine_tune(True)
        decoder_params = AttentionDecoderParams()
        decoder_params.attention_dim = args.attention_dim
        decoder_params.decoder_dim = args.decoder_dim
        decoder_params.embed_size = args.embed_size
        decoder_params.dropout = args.decoder_dropout
        decoder_params.vocab = vocab
        decoder_params.use_bert = args.use_bert
        decoder = AttentionDecoder(device, decoder_params)
        if args.use_glove:
            from embed import load_glove_vectors
            decoder.load_pretrained_embeddins(load_glove_vectors())
        decoder.fine_tune_embeddings(args.fine_tune_embedding)
        start_epoch, metrics, opt_state = 0, {}, None
    else:
        chkpt = load_checkpoint(device, args, weights_only=not getattr(args, 'trusted_checkpoint', False))
        start_epoch, enc_sd, dec_sd, enc_opt_state, opt_state, metrics = unpack_checkpoint(chkpt)
        # whole-module checkpoints (save_checkpoint(..., whole_modules=True), the reference's format)
        enc_sd, dec_sd, enc_opt_state, opt_state = (
            v.state_dict() if hasattr(v, 'state_dict') else v for v in (enc_sd, dec_sd, enc_opt_state, opt_state))
        start_epoch += 1
        encoder = EncoderAttention()
        encoder.load_state_dict(enc_sd)
        if args.fine_tune_encoder:
            encoder.fine_tune(True)
        decoder_params = AttentionDecoderParams()
        decoder_params.attention_dim, decoder_params.decoder_dim = args.attention_dim, args.decoder_dim
        decoder_params.embed_size, decoder_params.dropout = args.embed_size, args.decoder_dropout
        decoder_params.vocab = vocab
        decoder_params.use_bert = args.use_bert  # as the fresh-start branch (the pickle keeps it)
        decoder = AttentionDecoder(device, decoder_params)
        if dec_sd["embedding.weight"].dtype == torch.float64:
            decoder.load_pretrained_embeddins(dec_sd["embedding.weight"].clone())
        decoder.load_state_dict(dec_sd)
        decoder.fine_tune_embeddings(args.fine_tune_embedding)

    if args.use_bert:
        # the real BERT features (reference :96-100) from a LOCAL checkpoint: --bert_path, else
        # PathConfig.bert_dir when that directory exists; with neither, the first step raises as before
        from pathconf import PathConfig
        bert_path = getattr(args, 'bert_path', None)
        if bert_path is None and os.path.isdir(PathConfig.bert_dir):
            bert_path = PathConfig.bert_dir
        if bert_path is not None:
            from capmi.bert import build_embedder
            decoder.bert_embedder = build_embedder(decoder, bert_path, device)

    return encoder, decoder, start_epoch, metrics, opt_state, enc_opt_state


def train(device, args):
    """Trains the attention model (reference :287-452), same loop and log line.

    Differences, all deliberate: the step runs the fused capmi path (hoisted
    GEMMs, fused CE + regulariser, gradients written in place, clamp fused into
    Adam); ``loss.item()`` syncs only every ``print_freq`` batches; data-parallel
    over torchrun ranks when WORLD_SIZE > 1 (gradient all-reduce over RCCL);
    checkpoints hold state_dicts (Q13). ``args.image_cache_gb`` > 0 (HIP device, real COCO): the
    resized uint8 images stay on the device and each JPEG is decoded once per run
    (capmi.imagepipe.DeviceImageCache; the same image tensors, bit for bit)."""
    from capmi import dist as cdist
    from capmi.imagepipe import ImageFeeder, collate_images, image_cache_for
    from capmi.train_step import AttentionTrainStep

    ctx = cdist.init_from_env(device)
    device = ctx.device
    dataset = _train_dataset(args, device)
    pad_idx = dataset.vocab(PAD_TOKEN)

    def collate_fn(data):
        from torch.nn.utils.rnn import pad_sequence
        imgs, captions, *keys = zip(*data)
        # tensors are stacked; decoded uint8 images (COCODataset without a transform) are packed and resized
        # on the GPU, with their keys when the image cache is on
        imgs = collate_images(imgs, *keys)
        captions = pad_sequence(captions, batch_first=True, padding_value=pad_idx)
        caption_lengths = [len(caption) for caption in captions]  # after padding (Q1)
        return imgs, captions, caption_lengths

    sampler = cdist.sampler_for(dataset, ctx)
    # with the image cache the workers live for the whole run (they read the dataset's shared `present` flags):
    # later epochs then start no processes, which is all the host would have left to do in them
    train_loader = torch.utils.data.DataLoader(
        dataset=dataset, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler,
        num_workers=args.workers, collate_fn=collate_fn, pin_memory=True,
        persistent_workers=args.workers > 0 and getattr(dataset, "return_image_key", False))

    encoder, decoder, start_epoch, metrics, opt_state, enc_opt_state = _build_models(args, dataset.vocab, device)
    encoder = encoder.to(device)
    decoder = decoder.to(device)
    # every rank starts from rank 0's weights and BN buffers: without models/resnet101.pth the
    # (frozen) ResNet keeps a random init that would differ per rank
    cdist.broadcast_module(encoder, ctx)
    cdist.broadcast_module(decoder, ctx)
    decoder_optimizer = FusedAdam(filter(lambda p: p.requires_grad, decoder.parameters()),
                                  lr=args.decoder_lr)
    if opt_state is not None:
        decoder_optimizer.load_state_dict(opt_state)
    encoder_optimizer = None
    if args.fine_tune_encoder:
        encoder_optimizer = FusedAdam(filter(lambda p: p.requires_grad, encoder.parameters()),
                                      lr=args.encoder_lr)
        if args.checkpoint is not None and enc_opt_state is not None:
            encoder_optimizer.load_state_dict(enc_opt_state)
    # pipelined: the frozen encoder of batch k overlaps the decoder step of batch k-1
    # (bit-identical results; losses arrive one batch late and are logged in order).
    # Fine-tuning runs the sequential step (the encoder needs the previous update).
    # On HIP graphs (the launch mode bench.py measures): each (batch, caption length) shape is
    # captured once and replayed; ragged batches, and new shapes once CAPMI_GRAPH_CACHE shapes are
    # held, run eagerly. CAPMI_TRAIN_GRAPH=0: every step eager.
    on_gpu = device.type == "cuda"
    step = AttentionTrainStep(encoder, decoder, decoder_optimizer, ctx, alpha_c=args.alpha_c,
                              pipeline=on_gpu and encoder_optimizer is None,
                              graph=on_gpu and os.environ.get("CAPMI_TRAIN_GRAPH", "1") != "0",
                              encoder_optimizer=encoder_optimizer)
    train.last_step = step  # (tests: which launch mode ran)
    if args.workers > 0:  # the loader's pin-memory thread allocates while a step is being captured
        step.capture_error_mode = "thread_local"

    decoder.train()
    encoder.train()
    num_batches = len(train_loader)
    epoch_losses = metrics.get('epoch_losses', [])
    feed = ImageFeeder(device, image_cache_for(args, dataset, device, args.batch_size))
    train.last_image_cache = feed.cache  # (tests: its stats)
    for epoch in range(start_epoch, args.epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        batch_losses = []
        accum_loss = AccumulatingMetric()
        accum_time = AccumulatingMetric()
        start = time.time()
        pending = []
        for batch_idx, (imgs, captions, caption_lengths) in enumerate(train_loader):
            imgs = feed(imgs)  # to the device; PackedImages: Resize + ToTensor + Normalize there (capmi.imagepipe)
            captions = captions.to(device, non_blocking=True)
            clip_gradient(decoder_optimizer, args.grad_clip)
            if encoder_optimizer is not None:
                clip_gradient(encoder_optimizer, args.grad_clip)
            loss = step(imgs, captions, caption_lengths)
            if batch_idx == num_batches - 1 and step.pipeline:
                pending.append(loss)
                loss = step.flush()  # the epoch's last decoder step
            if loss is not None:
                pending.append(loss if step.pipeline else loss.detach().clone())
            if (batch_idx % args.print_freq == 0 or batch_idx == num_batches - 1) and pending:
                if device.type == "cuda":
                    torch.cuda.synchronize()  # losses live on the decoder stream
                    K.sk_check()  # stream-K hand-off invariant (raises on a timed-out hand-off)
                for l in torch.stack([p for p in pending if p is not None]).view(-1).tolist():
                    batch_losses.append(l)
                    accum_loss.update(l)
                pending = []
                accum_time.update(time.time() - start)
                if ctx.rank == 0:
                    print(f'Epoch {epoch+1}/{args.epochs}, Batch {batch_idx+1}/{num_batches}, '
                          f'Loss {accum_loss.avg():.4f}, Time: {accum_time.val:.4f}')
            start = time.time()
        epoch_losses.append(batch_losses)
        metrics = {'epoch_losses': epoch_losses}
        if ctx.rank == 0:
            save_checkpoint(args, epoch, encoder, decoder, encoder_optimizer, decoder_optimizer, metrics)
    if ctx.rank == 0:
        print(f'Model {args.model_name} finished training for {args.epochs} epochs.')


def check_self_critical_args(args):
    """What self-critical training of the attention captioner asks of the flags, before any data is loaded (the
    twin of models.baseline.check_self_critical_args)."""
    if not getattr(args, 'checkpoint', None):
        raise SystemExit('self-critical training continues from a cross-entropy trained model: give --checkpoint '
                         '(an attention state-dict checkpoint in ./checkpoints)')
    if args.fine_tune_encoder:
        raise NotImplementedError('self-critical training with --fine_tune_encoder True: the features are computed '
                                  'once per step, without a graph')
    if getattr(args, 'use_bert', False):
        raise NotImplementedError('self-critical training with --use_bert True: the sampler has no BERT features '
                                  'for the tokens it draws')
    if not 0 <= args.sc_max_len <= 63:
        raise SystemExit('--sc_max_len must be 0..63 (a sampled caption holds at most 64 words)')


def train_self_critical(device, args):
    """Self-critical training of a cross-entropy trained attention captioner (capmi.scst): the twin of
    models.baseline.train_self_critical on the same ``--sc_*`` fields. ``args.checkpoint`` is loaded as eval.py
    --model_type attention loads it (sizes read off the tensors), the CIDEr-D tables are built from the training
    set's ``references(k)`` grouped by image, and AttentionSelfCriticalStep runs over the distinct images of every
    batch. Loss, reward and (``sc_baseline`` greedy) the greedy reward stay on the device and are read every
    ``print_freq`` batches and at the epoch's end. train.py does not dispatch here yet."""
    from capmi.scst import AttentionSelfCriticalStep
    from eval import _attention_models
    from models.baseline import self_critical_data, self_critical_loop
    check_self_critical_args(args)
    ctx, device, base, dataset, refs = self_critical_data(device, args)
    _, enc_sd, dec_sd, _, _, _ = unpack_checkpoint(
        load_checkpoint(device, args, verbose=ctx.rank == 0, weights_only=not getattr(args, "trusted_checkpoint", False)))
    if hasattr(dec_sd, 'state_dict'):  # a whole-module checkpoint
        enc_sd, dec_sd = enc_sd.state_dict(), dec_sd.state_dict()
    encoder, decoder = _attention_models(args, enc_sd, dec_sd, dataset.vocab, device)
    self_critical_loop(args, ctx, device, base, dataset, refs, encoder, decoder, AttentionSelfCriticalStep,
                       train_self_critical)


def evaluate(device, args, encoder, decoder, val_loader=None):
    """Reference :454-567: one teacher-forced pass over the validation set (batch 1 in the
    reference), loss = CE over the packed rows + ((1 - sum_t alpha)^2).mean(), greedy argmax
    hypotheses and the START/END/PAD-stripped references, then caption scores.

    The forward runs on the capmi kernels (no grad). ``val_loader`` defaults to the reference's
    COCO 'val' loader (needs the dataset); caption scoring (metric.get_eval_score -> the
    reference's eval_func BLEU/METEOR/ROUGE/CIDEr) is attempted and skipped when unavailable:
    the returned dict then holds the losses, references and hypotheses."""
    from torch.nn.utils.rnn import pack_padded_sequence
    from metric import get_eval_score
    from vocabulary import END_TOKEN, START_TOKEN
    if val_loader is None:
        from dataset import COCODataset  # real COCO path (pycocotools, nltk, images)
        dataset = COCODataset(mode='val', caption_max_len=args.max_caption_length)
        pad_idx = dataset.vocab(PAD_TOKEN)

        def collate_fn(data):
            from torch.nn.utils.rnn import pad_sequence
            imgs, captions = list(zip(*data))[:2]
            captions = pad_sequence(captions, batch_first=True, padding_value=pad_idx)
            return torch.stack(imgs, dim=0), captions, [len(c) for c in captions]
        val_loader = torch.utils.data.DataLoader(dataset=dataset, batch_size=1, shuffle=True,
                                                 num_workers=1, collate_fn=collate_fn)
    vocab = decoder.vocab
    drop = {vocab(START_TOKEN), vocab(END_TOKEN), vocab(PAD_TOKEN)}
    references, hypotheses, losses = [], [], []
    accum_loss = AccumulatingMetric()
    decoder.eval()
    encoder.eval()
    num_batches = len(val_loader)
    start_time = time.time()
    with torch.no_grad():
        for batch_idx, (imgs, captions, caption_lengths) in enumerate(val_loader):
            imgs = imgs.to(device)
            captions = captions.to(device)
            scores, caps_sorted, decode_lengths, alphas = decoder(encoder(imgs), captions, caption_lengths)
            targets = caps_sorted[:, 1:]
            sp = pack_padded_sequence(scores, decode_lengths, batch_first=True).data
            tp = pack_padded_sequence(targets, decode_lengths, batch_first=True).data
            loss = nn.functional.cross_entropy(sp, tp) + ((1. - alphas.sum(dim=1)) ** 2).mean()
            accum_loss.update(loss.item(), sum(decode_lengths))
            losses.append(loss.item())
            for j in range(targets.shape[0]):
                ref = [w for w in targets[j].tolist() if w not in drop]
                references.append([ref for _ in targets[j].tolist()])  # reference :527-528
            preds = torch.max(scores, dim=2)[1].tolist()
            hypotheses.extend([[w for w in p[:decode_lengths[j]] if w not in drop] for j, p in enumerate(preds)])
            if batch_idx % args.print_freq == 0:
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
    """The validation pass of ``evaluate`` over ``batch_size`` captions per step, with per-caption
    results equal to what the reference computes one caption at a time (reference :454-567 at batch 1).

    ``dataset``: items ``(img, caption)`` or the val-mode 4-tuple; default the reference's COCO 'val' set
    (needs the dataset). Captions are taken in dataset order (no shuffle), padded to the batch maximum and
    passed with their true lengths. Per batch: one encoder forward, capmi.evalpass.TeacherForcedEval (loss,
    greedy tokens and top-1 / top-5 counts on the device), one asynchronous copy of the small result buffer
    to pinned host memory; the device is synchronised only every ``print_freq`` batches and at the end.

    Returns a JSON-serialisable dict: the capmi.scoring.caption_scores keys (BLEU-1..4, ROUGE-L, CIDEr; no
    METEOR), ``losses`` (per caption, dataset order), ``loss`` (their average weighted by decode length:
    the running figure of the reference's log line), ``top1_acc`` / ``top5_acc`` over all scored rows,
    ``references`` and ``hypotheses`` (built as the reference builds them at batch 1: the START/END/PAD-
    stripped target repeated once per target position of that caption, and the stripped greedy tokens)."""
    from torch.nn.utils.rnn import pad_sequence
    from capmi import evalpass
    from capmi.scoring import caption_scores
    from vocabulary import END_TOKEN, START_TOKEN
    if dataset is None:
        from dataset import COCODataset  # real COCO path (pycocotools, nltk, images)
        dataset = COCODataset(mode='val', caption_max_len=args.max_caption_length)
    vocab = decoder.vocab
    pad_idx = vocab(PAD_TOKEN)
    drop = {vocab(START_TOKEN), vocab(END_TOKEN), pad_idx}

    def collate_fn(data):
        imgs, captions = list(zip(*data))[:2]
        return (torch.stack(imgs, dim=0), pad_sequence(captions, batch_first=True, padding_value=pad_idx),
                [len(c) for c in captions])  # true lengths (evaluate's loader pads first: equal at batch 1)

    loader = torch.utils.data.DataLoader(dataset=dataset, batch_size=int(batch_size), shuffle=False,
                                         num_workers=int(getattr(args, "workers", 0) or 0), collate_fn=collate_fn)
    on_gpu = torch.device(device).type == "cuda"
    tf_eval = evalpass.TeacherForcedEval(decoder, alpha_c=1.0)  # the reference's validation loss: (1 - sum alpha)^2
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
            res = evalpass.unpack(host, len(lengths), T)
            loss_h, pred_h = res["cap_loss"].tolist(), res["pred"].tolist()
            hits1 += int(res["top1"].sum())
            hits5 += int(res["top5"].sum())
            for i, n in enumerate(lengths):
                dl = n - 1
                accum_loss.update(loss_h[i], dl)
                losses.append(loss_h[i])
                rows += dl
                ref = [w for w in caps_h[i][1:n] if w not in drop]
                references.append([ref for _ in range(dl)])  # reference :527-528, at this caption's own length
                hypotheses.append([w for w in pred_h[i][:dl] if w not in drop])
        del pending[:]

    with torch.no_grad():
        for batch_idx, (imgs, captions, caption_lengths) in enumerate(loader):
            imgs = imgs.to(device, non_blocking=True)
            res = tf_eval(encoder(imgs), captions.to(device, non_blocking=True), caption_lengths)
            packed = res["packed"]
            host = torch.empty(packed.shape, dtype=packed.dtype, pin_memory=on_gpu)
            host.copy_(packed, non_blocking=True)
            pending.append((host, captions.tolist(), caption_lengths, res["pred"].shape[1]))
            if batch_idx % args.print_freq == 0:
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
    """Validation on generated captions (capmi.genval): every image of ``dataset`` (default the COCO 'val' set) is
    captioned once by ``BatchedBeamSearch`` with ``args.beam_size`` beams (default 3), at most
    ``args.max_decode_len`` words (default 50, at most 63) and the length normalisation ``args.length_alpha``
    (default 0: the raw beam score), and scored against all of its references. Captions, counting and CIDEr-D
    rows stay on the device; the host synchronises every ``print_freq`` batches and at the end.

    Returns a JSON-serialisable dict: the capmi.scoring.caption_scores keys, ``hypotheses`` (token ids per image,
    in image order, START / END / PAD stripped), ``image_keys``, ``unfinished`` (images without a finished beam:
    their best live beam is scored), ``mean_length``, ``host_syncs`` (the searches' ``sync_every`` reads) and
    ``captions_per_s`` (over everything from the reference tables' build to the scores). ``max_decode_len`` above 63
    is a ``ValueError``."""
    from capmi import genval
    from capmi.beam import BatchedBeamSearch
    if torch.device(device).type != "cuda":
        raise RuntimeError("generated-caption validation runs on a HIP device (the search and the scores are kernels)")
    if dataset is None:
        from dataset import COCODataset  # real COCO path (pycocotools, nltk, images)
        dataset = COCODataset(mode='val', caption_max_len=getattr(args, "max_caption_length", -1))
    search = BatchedBeamSearch(decoder, int(getattr(args, "beam_size", 3)))
    return genval.evaluate_generated(device, args, encoder, decoder, search, dataset, decoder.vocab, batch_size)


__all__ = ["SoftAttention", "AttentionDecoderParams", "AttentionDecoder", "train", "train_self_critical", "evaluate",
           "evaluate_batched", "evaluate_generated"]
