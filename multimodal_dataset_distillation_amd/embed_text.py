"""Writes a caption-embedding cache with the frozen CLIP text tower: the reference's `textprocess` (file_type `text`, the
test captions) and `textprocess_train` (file_type `train_text`, the training pairs' captions) for `--text_encoder clip`
(reference distill.py:107-144, networks.py:700-726).

    python -m multimodal_dataset_distillation_amd.embed_text --dataset flickr --file_type train_text \\
        --tokens train_ids.npy --clip_weights clip_vit_b32_state.pt [--embed_dir DIR] [--chunk 2000] [--compute_dtype bf16]

--tokens: an int array [n, 77] of `clip.tokenize` ids (.npy; or .npz / .pt with the key `tokens`).  --clip_weights: a
`torch.save`d state dict of the CLIP model (`clip.load("ViT-B/32")[0].state_dict()`): the text tower's entries are taken
by name, `visual.*` and `logit_scale` are ignored.  The result is `{dataset}_clip_{file_type}_embed.npz`, which
embed_cache.load_embed_cache reads.

--captions FILE (one caption per line) tokenises with `clip.tokenize` when the `clip` package can be imported; nothing
else here needs that package.
"""
import argparse

import numpy as np
import torch

from .embed_cache import load_tensor_file, write_embed_cache
from .text_tower import VARIANTS, TextTower


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--file_type", required=True, choices=["text", "train_text"])
    ap.add_argument("--text_encoder", default="clip", choices=["clip"], help="bert is not built")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--tokens", help="int [n, context] token ids: .npy, or .npz / .pt with the key 'tokens'")
    src.add_argument("--captions", help="text file, one caption per line (needs the `clip` package for clip.tokenize)")
    ap.add_argument("--clip_weights", required=True, help="torch.save'd state dict of the CLIP model")
    ap.add_argument("--embed_dir", default=".")
    ap.add_argument("--chunk", type=int, default=2000, help="sequences per call (the reference's train chunk)")
    ap.add_argument("--compute_dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--variant", default="clip_text_b32", choices=list(VARIANTS))
    return ap


def _tokenize(path, context):
    try:
        import clip
    except ImportError as e:
        raise SystemExit("--captions needs the `clip` package for clip.tokenize (%s); pass --tokens instead" % e)
    with open(path) as f:
        texts = [line.rstrip("\n") for line in f]
    return clip.tokenize(texts, context_length=context)


def main(args):
    if args.chunk < 1:
        raise ValueError("--chunk must be at least 1")
    tower = TextTower(args.variant, max_batch=args.chunk, compute_dtype=args.compute_dtype)
    try:
        ids = load_tensor_file(args.tokens, key="tokens") if args.tokens else _tokenize(args.captions, tower.context)
        ids = tower.check_ids(ids)
        tower.load_state_dict_file(args.clip_weights)
        emb = tower.encode(ids).cpu()
    finally:
        tower.close()
    path = write_embed_cache(args, args.file_type, emb, args.embed_dir)
    print("wrote %s: %s float32 (%s, %s)" % (path, tuple(emb.shape), args.variant, args.compute_dtype))
    return path


if __name__ == "__main__":
    main(build_parser().parse_args())
