"""Caption generation with beam search (reference gen_captions.py:16-131), same function name and
signature. On a HIP device the decode runs on capmi's kernels (capmi.beam.BeamSearch); the
encoder is the capmi EncoderAttention. Image loading / plotting of the reference's CLI
(imageio, matplotlib, checkpoints of whole modules) is outside the built path.
``caption_images_beam_search`` is the batched form (capmi.beam.BatchedBeamSearch): B images per call.
``caption_images_sample`` / ``baseline_caption_images_sample`` draw captions from the model's own distribution
instead (capmi.sample): several per image, each with the log-probability of every token."""
import torch

from capmi.beam import BaselineBatchedBeamSearch, BatchedBeamSearch, BeamSearch
from capmi.sample import BaselineBatchedSampler, BatchedSampler
from vocabulary import END_TOKEN, START_TOKEN


def attention_caption_image_beam_search(device, args, img, encoder, decoder, vocab):
    """Reads an image and captions it with beam search (reference :16-131).

    Returns (caption token ids, attention weights (steps+1, 14, 14) as nested lists, finished)."""
    with torch.no_grad():
        encoder_out = encoder(img)  # (1, 14, 14, 2048)
    return BeamSearch(decoder, args.beam_size).search(encoder_out, vocab(START_TOKEN), vocab(END_TOKEN))


def caption_images_beam_search(device, args, imgs, encoder, decoder, vocab):
    """Captions a batch of images (B, 3, H, W) with beam search: one encoder forward for the batch, then
    the batched beam search with its beam state on the device.

    Returns a list of B tuples (caption token ids, attention weights (steps+1, 14, 14), finished), each
    what ``attention_caption_image_beam_search`` returns for that image alone."""
    with torch.no_grad():
        encoder_out = encoder(imgs)  # (B, 14, 14, 2048)
    return BatchedBeamSearch(decoder, args.beam_size).search(encoder_out, vocab(START_TOKEN), vocab(END_TOKEN))


def baseline_caption_images_beam_search(device, args, imgs, encoder, decoder, vocab):
    """Captions a batch of images (B, 3, H, W) with the baseline model: one ``Encoder`` forward for the batch,
    then capmi.beam.BaselineBatchedBeamSearch.

    Returns a list of B tuples (caption token ids, [], finished); failure: ([start, end], [], False)."""
    with torch.no_grad():
        img_features = encoder(imgs)  # (B, embed_size)
    return BaselineBatchedBeamSearch(decoder, args.beam_size).search(img_features, vocab(START_TOKEN),
                                                                     vocab(END_TOKEN))


def _sample_args(args):
    return (getattr(args, "num_samples", 1), getattr(args, "temperature", 1.0), getattr(args, "top_k", 0),
            getattr(args, "seed", None))


def caption_images_sample(device, args, imgs, encoder, decoder, vocab):
    """Draws ``args.num_samples`` captions per image of a batch (B, 3, H, W) from the attention captioner at
    ``args.temperature`` (0: the greedy rollout) over the ``args.top_k`` likeliest words (0: all), the uniforms
    seeded with ``args.seed``; an absent attribute means 1, 1.0, 0 and None (a fresh seed).

    Returns a list of B lists of num_samples dicts {seq, token_logp, logp, finished, alphas} (capmi.sample)."""
    n, temperature, top_k, seed = _sample_args(args)
    with torch.no_grad():
        encoder_out = encoder(imgs)  # (B, 14, 14, 2048)
    return BatchedSampler(decoder, n, temperature, top_k).sample(encoder_out, vocab(START_TOKEN), vocab(END_TOKEN),
                                                                 seed=seed)


def baseline_caption_images_sample(device, args, imgs, encoder, decoder, vocab):
    """``caption_images_sample`` for the baseline model: one ``Encoder`` forward for the batch, then
    capmi.sample.BaselineBatchedSampler. The dicts' ``alphas`` are empty."""
    n, temperature, top_k, seed = _sample_args(args)
    with torch.no_grad():
        img_features = encoder(imgs)  # (B, embed_size)
    return BaselineBatchedSampler(decoder, n, temperature, top_k).sample(img_features, vocab(START_TOKEN),
                                                                         vocab(END_TOKEN), seed=seed)
