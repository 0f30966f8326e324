"""Evaluation entry point with the reference CLI (eval.py:21-45).

    python eval.py basic_att_0.pth.tar --model_type attention [--batch_size 64]
    python eval.py basic_att_0.pth.tar --model_type attention --batch_size 64 --synthetic_size 512
    python eval.py baseline_0.pth.tar --model_type baseline --batch_size 64 --synthetic_size 512
    python eval.py basic_att_0.pth.tar --model_type attention --batch_size 64 --decode beam --beam_size 3

The reference's arguments are kept: ``checkpoint`` (a file in ./checkpoints), ``--model_type``,
``--max_caption_length``, ``--print_freq``. Added: ``--batch_size`` (1, the default, runs the reference's
one-caption-at-a-time ``evaluate``; larger runs ``evaluate_batched`` of models.attention / models.baseline,
whose per-caption numbers are the same),``--synthetic_size`` / ``--vocab_size`` / ``--synthetic_len`` (COCO-shaped synthetic
captions of ragged lengths instead of the COCO 'val' set), ``--scorer device`` (the batched pass counts BLEU /
ROUGE-L / CIDEr on the HIP device, capmi.devscore; ``host``, the default, is capmi.scoring) and
``--trusted_checkpoint`` (as train.py: the reference's whole-module checkpoints are pickles). ``--decode beam``
(with ``--beam_size``, ``--max_decode_len``, ``--length_alpha``) replaces the teacher-forced pass by validation on
generated captions (capmi.genval): every image captioned once by beam search and scored against all of its references
on the HIP device, for either ``--model_type``. The metrics are
printed and written to <PathConfig.eval_data>/<checkpoint stem>.json.
"""
import argparse
import json
import os
import sys

sys.path.append('cocoapi/PythonAPI/')
import torch  # noqa: E402

from checkpoint import load_checkpoint, unpack_checkpoint  # noqa: E402
from pathconf import PathConfig  # noqa: E402


def save_eval_data(name, d):
    os.makedirs(PathConfig.eval_data, exist_ok=True)
    path = os.path.join(PathConfig.eval_data, f'{name}.json')
    with open(path, 'w') as f:
        json.dump(d, f)
    return path


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Evaluation')
    parser.add_argument('checkpoint', type=str, help='checkpoint of trained model.')
    parser.add_argument('--model_type', type=str, choices=['baseline', 'attention'], help='type of model to evaluate')
    parser.add_argument('--max_caption_length', type=int, default=-1,
                        help='only use captions with caption length <= 50 when training.')
    parser.add_argument('--print_freq', type=int, default=1, help='print training/validation stats every __ batches.')
    # capmi additions
    parser.add_argument('--batch_size', type=int, default=1,
                        help='captions per step; 1 is the reference loop, > 1 the batched pass.')
    parser.add_argument('--synthetic_size', type=int, default=0,
                        help='evaluate on this many synthetic ragged captions instead of COCO val.')
    parser.add_argument('--vocab_size', type=int, default=8100, help='synthetic vocabulary size.')
    parser.add_argument('--synthetic_len', type=int, default=25, help='longest synthetic caption.')
    parser.add_argument('--trusted_checkpoint', type=bool, default=False,
                        help='checkpoint is a whole-module pickle you wrote yourself (load with weights_only=False).')
    parser.add_argument('--scorer', type=str, default='host', choices=['host', 'device'],
                        help='where the batched pass scores its captions: capmi.scoring on the host or '
                             'capmi.devscore on the HIP device.')
    parser.add_argument('--decode', type=str, default='teacher', choices=['teacher', 'beam'],
                        help='teacher: the teacher-forced pass. beam: every image captioned once by beam search and '
                             'scored against all of its references on the HIP device (capmi.genval).')
    parser.add_argument('--beam_size', type=int, default=3, help='beams per image of --decode beam.')
    parser.add_argument('--max_decode_len', type=int, default=50,
                        help='longest caption of --decode beam, in words (at most 63).')
    parser.add_argument('--length_alpha', type=float, default=0.0,
                        help='--decode beam picks the finished beam with the largest score / length^alpha '
                             '(0: the raw score, as gen_captions.py).')
    args = parser.parse_args(argv)
    if args.batch_size < 1:
        parser.error('--batch_size must be >= 1')
    return args


def _synthetic_dataset(args):
    from capmi.data import SyntheticCOCO
    return SyntheticCOCO(args.synthetic_size, V=args.vocab_size, L=args.synthetic_len, ragged=True)


def _attention_models(args, enc_sd, dec_sd, vocab, device):
    """Modules for a state_dict checkpoint; the decoder's sizes are read off its tensors."""
    from models.attention import AttentionDecoder, AttentionDecoderParams
    from models.encoder import EncoderAttention
    encoder = EncoderAttention()
    encoder.load_state_dict(enc_sd)
    prm = AttentionDecoderParams()
    prm.attention_dim = dec_sd["attention.enc_att.weight"].shape[0]
    prm.decoder_dim = dec_sd["decode_step.weight_hh"].shape[1]
    prm.embed_size = dec_sd["decode_step.weight_ih"].shape[1] - dec_sd["attention.enc_att.weight"].shape[1]
    prm.vocab = vocab
    if len(vocab) != dec_sd["fc.weight"].shape[0]:
        raise SystemError(f'checkpoint decodes {dec_sd["fc.weight"].shape[0]} words, the vocabulary has {len(vocab)}')
    decoder = AttentionDecoder(device, prm)
    if dec_sd["embedding.weight"].dtype == torch.float64:  # GloVe tables stay fp64
        decoder.load_pretrained_embeddins(dec_sd["embedding.weight"].clone())
    decoder.load_state_dict(dec_sd)
    return encoder.to(device), decoder.to(device)


def _baseline_models(args, enc_sd, dec_sd, device):
    """Modules for a baseline state_dict checkpoint; every size is read off the tensors."""
    from models.baseline import BaselineDecoder, BaselineDecoderParams
    from models.encoder import Encoder
    if args.synthetic_size > 0:
        n_vocab = args.vocab_size
    else:
        if not os.path.exists(PathConfig.vocab_file):
            raise SystemError('Must run "python init.py --vocab True" before evaluating.')
        from vocabulary import load_vocab
        n_vocab = len(load_vocab())
    if n_vocab != dec_sd["linear.weight"].shape[0]:
        raise SystemError(f'checkpoint decodes {dec_sd["linear.weight"].shape[0]} words, the vocabulary has {n_vocab}')
    encoder = Encoder(enc_sd["embed.weight"].shape[0])
    encoder.load_state_dict(enc_sd)
    prm = BaselineDecoderParams()
    prm.embed_size = dec_sd["embedding.weight"].shape[1]
    prm.hidden_size = dec_sd["lstm.weight_hh_l0"].shape[1]
    prm.vocab_size = dec_sd["linear.weight"].shape[0]
    decoder = BaselineDecoder(prm)
    if dec_sd["embedding.weight"].dtype == torch.float64:  # GloVe tables stay fp64
        decoder.load_pretrained_embeddins(dec_sd["embedding.weight"].clone())
    decoder.load_state_dict(dec_sd)
    return encoder.to(device), decoder.to(device)


def main(argv=None):
    args = parse_args(argv)
    device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    chkpt = load_checkpoint(device, args, weights_only=not args.trusted_checkpoint)
    _, encoder, decoder, _, _, _ = unpack_checkpoint(chkpt)
    name = os.path.basename(args.checkpoint).split('.')[0]

    if args.model_type == 'baseline':
        from models.baseline import evaluate as evaluate_baseline_model
        if not hasattr(decoder, 'state_dict'):  # state_dict checkpoint (the default format)
            encoder, decoder = _baseline_models(args, encoder, decoder, device)
        else:
            encoder, decoder = encoder.to(device), decoder.to(device)
        if args.decode == 'beam':
            from models.baseline import evaluate_generated
            metrics = evaluate_generated(device, args, encoder, decoder, batch_size=args.batch_size)
        else:
            metrics = evaluate_baseline_model(device, args, encoder, decoder)
    elif args.model_type == 'attention':
        from models.attention import evaluate as evaluate_attention_model, evaluate_batched
        dataset = _synthetic_dataset(args) if args.synthetic_size > 0 else None
        if not hasattr(decoder, 'state_dict'):  # state_dict checkpoint (the default format)
            if dataset is not None:
                vocab = dataset.vocab
            else:
                if not os.path.exists(PathConfig.vocab_file):
                    raise SystemError('Must run "python init.py --vocab True" before evaluating.')
                from vocabulary import load_vocab
                vocab = load_vocab()
            encoder, decoder = _attention_models(args, encoder, decoder, vocab, device)
        else:
            encoder, decoder = encoder.to(device), decoder.to(device)
        if args.decode == 'beam':
            from models.attention import evaluate_generated
            metrics = evaluate_generated(device, args, encoder, decoder, dataset=dataset, batch_size=args.batch_size)
        elif args.batch_size > 1:
            metrics = evaluate_batched(device, args, encoder, decoder, dataset=dataset, batch_size=args.batch_size)
        else:
            metrics = evaluate_attention_model(device, args, encoder, decoder, val_loader=_loader_1(dataset, decoder))
    else:
        raise SystemExit('--model_type must be baseline or attention')
    print({k: v for k, v in metrics.items() if k not in ('references', 'hypotheses', 'losses', 'image_keys')})
    path = save_eval_data(name, metrics)
    print(f'Saved evaluation data to {path}')
    return metrics


def _loader_1(dataset, decoder):
    """Batch-1 loader over a synthetic set for ``evaluate`` (None: its own COCO 'val' loader)."""
    if dataset is None:
        return None
    from vocabulary import PAD_TOKEN
    pad_idx = decoder.vocab(PAD_TOKEN)

    def collate_fn(data):
        from torch.nn.utils.rnn import pad_sequence
        imgs, captions = list(zip(*data))[:2]
        captions = pad_sequence(captions, batch_first=True, padding_value=pad_idx)
        return torch.stack(imgs, dim=0), captions, [len(c) for c in captions]
    return torch.utils.data.DataLoader(dataset=dataset, batch_size=1, shuffle=False, num_workers=0,
                                       collate_fn=collate_fn)


if __name__ == '__main__':
    main()
