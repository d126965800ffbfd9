#!/usr/bin/env python3
"""Classify your own images with a trained checkpoint: a labelled support folder becomes a PrototypeBank, a query folder is scored against it.

  python -m fewshot_vit_amd.predict --load ckpt.pth --support support/ --query query/ --out preds.csv

`--support DIR` holds one sub-folder per class with any number of images each; classes are numbered in sorted folder order.  `--query DIR` is a
flat folder of images or class sub-folders of the same names (then the accuracy is printed).  Images are decoded and transformed as by the
'image-folder' dataset (Resize(box) -> CenterCrop(size) with Pillow, normalisation on the device).  `--save-bank F` stores the bank (class sums,
counts, method, class names); `--load-bank F` restores one, and together with `--support` extends it with further examples of the same classes
without re-encoding the earlier ones.  The CSV has one row per query image: file, pred_class (the class number), logit_0 .. logit_{way-1}.
With `--topk K` (1 <= K <= 32) only the K best classes of every image are formed - the full logits are neither computed nor stored, which is what a
bank of tens of thousands of classes needs - and the row is file, pred_class, pred_name, then class_i, name_i, logit_i, prob_i for i = 0 .. K-1 in
descending order (ties: the lower class); prob is the softmax probability over all classes; a rank beyond the number of classes holds class -1.

`--head deepemd` scores with the DeepEMD head of a SUN-D checkpoint instead (models.deepemd, whole-image token maps): the support folder becomes a
TokenBank of class token maps (the mean map of a class), `--temperature T` is the head's temperature, and `--encoder NAME` names the encoder when
the checkpoint carries no `model_args`.  Without `--topk` every query is scored against every class; with `--topk K` only a shortlist of
`--shortlist M` classes (default min(32, classes), K <= M <= 32), drawn by the cosine of token means, is scored exactly, and prob is the softmax over
that shortlist.  A stored bank records its head and loads only under the same one.  The CSV columns are the same."""
import argparse
import csv
import os

import torch

from . import models
from .datasets.folder_datasets import ImageFolder
from .episodic import head_temp
from .models.emd_bank import TokenBank
from .models.proto_bank import PrototypeBank


def _listdir(path):
    return sorted(n for n in os.listdir(path) if not n.startswith('.'))


def class_folders(root):
    """sorted sub-folder names of root ([] when it is a flat folder of files)"""
    return [n for n in _listdir(root) if os.path.isdir(os.path.join(root, n))]


def list_labelled(root, classes):
    """-> (paths, labels) of root/<class>/<file> with labels indexing `classes`; a folder that is not in `classes` is an error"""
    paths, labels = [], []
    for c in class_folders(root):
        if c not in classes:
            raise ValueError(f'{root}: class folder {c!r} is not one of the bank\'s classes {classes}')
        for n in _listdir(os.path.join(root, c)):
            paths.append(os.path.join(root, c, n))
            labels.append(classes.index(c))
    return paths, labels


def encode_files(model, paths, image_size, box_size, device, batch=1024):
    """features [len(paths), out_dim] of the files through the eval engine, `batch` images decoded and uploaded at a time"""
    ds = ImageFolder.from_files(paths, [0] * len(paths), image_size, box_size, device, cache_bytes=0)      # every file is read once
    engine = model.encoder.engine()
    out = torch.empty(len(paths), engine.out_dim, dtype=torch.float32, device=device)
    for i in range(0, len(paths), batch):
        engine.forward(ds.gather(list(range(i, min(i + batch, len(paths))))), out=out[i:i + batch])
    return out


def load_model(path, method=None, numerics=None):
    model = models.load(torch.load(path, map_location='cpu'))
    if method is not None:
        model.method = method
    if numerics is not None:
        model.encoder.numerics = numerics
    return model


def encode_file_maps(model, paths, image_size, box_size, device, batch=1024):
    """token maps [len(paths), N, C] of the files through a DeepEMD model's encoder, `batch` images decoded and uploaded at a time"""
    ds = ImageFolder.from_files(paths, [0] * len(paths), image_size, box_size, device, cache_bytes=0)      # every file is read once
    return torch.cat([model._encode_eval(ds.gather(list(range(i, min(i + batch, len(paths))))), 'predict') for i in range(0, len(paths), batch)])


def load_deepemd(path, encoder=None, numerics=None, temperature=12.5):
    """A DeepEMD model around the encoder of a SUN-D (or pre-training) checkpoint: the encoder is the checkpoint's `model_args` one, else `encoder`"""
    from .models import deepemd
    ck = torch.load(path, map_location='cpu')
    margs = ck.get('model_args') if isinstance(ck, dict) else None
    if margs is not None:
        encoder, encoder_args = margs['encoder'], dict(margs.get('encoder_args', {}))
    elif encoder is None:
        raise SystemExit('predict: the checkpoint has no model_args; name its encoder with --encoder NAME')
    else:
        encoder_args = {}
    model = models.make('deepemd', encoder=encoder, encoder_args=encoder_args, temperature=temperature)
    model.load_state_dict(deepemd.encoder_state_dict(ck, set(model.state_dict().keys())), strict=True)
    if numerics is not None:
        model.encoder.numerics = numerics
    return model


def make_parser():
    p = argparse.ArgumentParser(prog='python -m fewshot_vit_amd.predict', description=__doc__.split('\n\n')[0])
    p.add_argument('--load', required=True, metavar='CKPT', help="a 'meta-baseline' checkpoint (the training drivers' schema); with --head deepemd a SUN-D checkpoint")
    p.add_argument('--support', metavar='DIR', help='labelled support set: one sub-folder per class')
    p.add_argument('--query', metavar='DIR', help='images to classify: a flat folder, or class sub-folders (prints the accuracy)')
    p.add_argument('--method', choices=['cos', 'sqr'], default=None, help="default: the checkpoint's")
    p.add_argument('--numerics', default=None, choices=[None, 'bf16', 'f16', 'bf16x2', 'f16x2', 'parity'], help="default: FSVIT_NUMERICS or 'bf16'")
    p.add_argument('--out', metavar='preds.csv', help='file,pred_class,logit_0.. per query image (with --topk: file,pred_class,pred_name,class_0,name_0,logit_0,prob_0,..)')
    p.add_argument('--topk', type=int, default=None, metavar='K', help='keep only the K best classes per image, 1..32, with their probabilities: no full logits')
    p.add_argument('--head', choices=['proto', 'deepemd'], default='proto', help="proto: cosine / distance to class prototypes; deepemd: the DeepEMD head of a SUN-D checkpoint")
    p.add_argument('--shortlist', type=int, default=None, metavar='M', help='--head deepemd with --topk K: score exactly only the M best classes by the cosine of token means, K <= M <= 32 (default min(32, classes))')
    p.add_argument('--temperature', type=float, default=12.5, metavar='T', help='--head deepemd: the temperature of the head')
    p.add_argument('--encoder', default=None, metavar='NAME', help='--head deepemd: the encoder of a checkpoint without model_args')
    p.add_argument('--save-bank', metavar='F', help='store the bank (of prototypes, or with --head deepemd of class token maps) after --support was added')
    p.add_argument('--load-bank', metavar='F', help='start from a stored bank; with --support: extend it')
    p.add_argument('--image-size', type=int, default=None, help="default: the encoder's input size")
    p.add_argument('--box-size', type=int, default=None, help='Resize target before the centre crop (default: image size * 8 / 7, the 256 -> 224 ratio)')
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    if not args.support and not args.load_bank:
        raise SystemExit('predict: give --support DIR, --load-bank F or both')
    if args.topk is not None and not 1 <= args.topk <= 32:
        raise SystemExit('predict: --topk K needs 1 <= K <= 32')
    deepemd = args.head == 'deepemd'
    if args.shortlist is not None and not (deepemd and args.topk is not None and args.topk <= args.shortlist <= 32):
        raise SystemExit('predict: --shortlist M goes with --head deepemd --topk K and needs K <= M <= 32')
    if not torch.cuda.is_available():
        raise RuntimeError('fsvit: predict needs an MI355X (no CPU fallback)')
    device = torch.device('cuda', torch.cuda.current_device())
    if deepemd:
        model = load_deepemd(args.load, args.encoder, args.numerics, args.temperature).to(device).eval()
        encode = encode_file_maps
    else:
        model = load_model(args.load, args.method, args.numerics).to(device).eval()
        encode = encode_files
    size = args.image_size or model.encoder.cfg['img_size']
    box = args.box_size or (size * 8) // 7
    bank, classes = None, None
    if args.load_bank:
        saved = torch.load(args.load_bank, map_location='cpu')
        if saved.get('head', 'proto') != args.head:               # (a file from before the flag holds a prototype bank)
            raise ValueError(f"{args.load_bank} holds a bank of --head {saved.get('head', 'proto')}, this run scores with --head {args.head}")
        classes = list(saved['classes'])
        bank = (TokenBank if deepemd else PrototypeBank).from_state_dict(saved['bank'], device)
        if not deepemd and bank.method != model.method:
            raise ValueError(f'{args.load_bank} was built for {bank.method!r}, the model scores with {model.method!r}')
    if args.support:
        if classes is None:
            classes = class_folders(args.support)
            if not classes:
                raise ValueError(f'{args.support}: no class sub-folders')
        paths, labels = list_labelled(args.support, classes)
        feat = encode(model, paths, size, box, device)
        if bank is None:
            bank = TokenBank(len(classes), feat.shape[1], feat.shape[2], device) if deepemd else PrototypeBank(len(classes), feat.shape[1], model.method, device)
        bank.add(feat, torch.tensor(labels, dtype=torch.int64, device=device)).check()
    print('bank: {} classes, {} support images ({})'.format(len(classes), int(bank.counts.sum()), 'deepemd' if deepemd else bank.method))
    if args.save_bank:
        torch.save({'bank': {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in bank.state_dict().items()}, 'classes': classes,
                    'head': args.head}, args.save_bank)
    out = {'bank': bank, 'classes': classes}
    if args.query:
        sub = class_folders(args.query)
        if sub:
            paths, truth = list_labelled(args.query, classes)
        else:
            paths, truth = [os.path.join(args.query, n) for n in _listdir(args.query)], None
        feat = encode(model, paths, size, box, device)
        temp = model.temperature if deepemd else head_temp(model, on_device=True)
        if args.topk is not None:
            top = bank.topk(feat, args.topk, temp, args.shortlist) if deepemd else bank.topk(feat, args.topk, temp)
            top_c, top_l, top_p = (t.cpu() for t in top)
            pred = top_c[:, 0]
            out.update(files=paths, pred=pred, topk_classes=top_c, topk_logits=top_l, topk_prob=top_p)
        else:
            if deepemd:
                logits = bank.logits(feat, temp)
                pred = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, 0]            # the first maximum of every row
            else:
                pred, logits = bank.predict(feat, temp)
            pred, logits = pred.cpu(), logits.cpu()
            out.update(files=paths, pred=pred, logits=logits)
        if deepemd:
            from .models.deepemd import check_status_count
            check_status_count(bank.status_count)
        if truth is not None:
            out['acc'] = float((pred == torch.tensor(truth)).double().mean()) if paths else float('nan')
            print('accuracy: {:.2f} % over {} images'.format(out['acc'] * 100, len(paths)))
        if args.out:
            with open(args.out, 'w', newline='') as f:
                w = csv.writer(f)
                if args.topk is not None:
                    name = lambda c: classes[c] if c >= 0 else ''
                    w.writerow(['file', 'pred_class', 'pred_name'] + [f'{h}_{i}' for i in range(args.topk) for h in ('class', 'name', 'logit', 'prob')])
                    for p, cs, ls, ps in zip(paths, top_c.tolist(), top_l.tolist(), top_p.tolist()):
                        w.writerow([p, cs[0], name(cs[0])] + [x for c, l, pr in zip(cs, ls, ps) for x in (c, name(c), repr(l), repr(pr))])
                else:
                    w.writerow(['file', 'pred_class'] + [f'logit_{c}' for c in range(len(classes))])
                    for p, c, row in zip(paths, pred.tolist(), logits.tolist()):
                        w.writerow([p, c] + [repr(v) for v in row])
    return out


if __name__ == '__main__':
    main()
