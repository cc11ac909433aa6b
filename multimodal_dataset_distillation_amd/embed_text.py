"""Writes a caption-embedding cache with a frozen text tower: the reference's `textprocess` (file_type `text`, the test
captions) and `textprocess_train` (file_type `train_text`, the training pairs' captions) for `--text_encoder clip` and
`--text_encoder bert` (reference distill.py:107-144, networks.py:700-735).

    python -m multimodal_dataset_distillation_amd.embed_text --dataset flickr --file_type train_text \\
        --tokens train_ids.npy --clip_weights clip_vit_b32_state.pt [--embed_dir DIR] [--chunk 2000] [--compute_dtype bf16]

--tokens: an int array [n, 77] of `clip.tokenize` ids (.npy; or .npz / .pt with the key `tokens`).  --clip_weights: a
`torch.save`d state dict of the CLIP model (`clip.load("ViT-B/32")[0].state_dict()`): the text tower's entries are taken
by name, `visual.*` and `logit_scale` are ignored.  The result is `{dataset}_clip_{file_type}_embed.npz`, which
embed_cache.load_embed_cache reads.

--captions FILE (one caption per line) tokenises with `clip.tokenize` when the `clip` package can be imported; nothing
else here needs that package.

    python -m multimodal_dataset_distillation_amd.embed_text --text_encoder bert --dataset flickr --file_type train_text \
        --tokens train_tokens.npz --bert_weights bert_base_uncased_state.pt [--chunk 2000] [--max_tokens 65536] ...

--text_encoder bert: --tokens is an .npz / .pt with the key `tokens` (int [n, L], L <= 512: `input_ids` of
`BertTokenizer.batch_encode_plus(padding=True, truncation=True)`) and optionally `attention_mask` (without it the mask is
`tokens != 0`), or an .npy of the ids.  --bert_weights: a `torch.save`d state dict of `BertModel` (keys bare or under
`bert.`; `pooler.*` and `cls.*` are ignored).  The variant defaults to `bert_base_uncased`, the result is
`{dataset}_bert_{file_type}_embed.npz` (768-d: `last_hidden_state[:, 0]`).  The tokens are packed -- no padded row is
computed -- and a call takes at most --chunk captions and --max_tokens token rows.  --captions FILE --vocab vocab.txt
tokenises with `transformers.BertTokenizer(vocab_file, do_lower_case=True)` when that package can be imported; the
vocabulary file is the user's, nothing is fetched.
"""
import argparse

import numpy as np
import torch

from .embed_cache import load_tensor_file, write_embed_cache
from .text_tower import BERT_VARIANTS, CLIP_VARIANTS, VARIANTS, TextTower

DEFAULT_VARIANT = {"clip": "clip_text_b32", "bert": "bert_base_uncased"}


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--file_type", required=True, choices=["text", "train_text"])
    ap.add_argument("--text_encoder", default="clip", choices=["clip", "bert"])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--tokens", help="int [n, context] token ids: .npy, or .npz / .pt with the key 'tokens' (bert: and "
                                      "optionally 'attention_mask')")
    src.add_argument("--captions", help="text file, one caption per line (clip: needs the `clip` package for clip.tokenize; "
                                        "bert: needs `transformers` and --vocab)")
    ap.add_argument("--clip_weights", help="torch.save'd state dict of the CLIP model (required for --text_encoder clip)")
    ap.add_argument("--bert_weights", help="torch.save'd state dict of BertModel (required for --text_encoder bert)")
    ap.add_argument("--vocab", help="bert --captions: the WordPiece vocabulary file (vocab.txt) of the model")
    ap.add_argument("--embed_dir", default=".")
    ap.add_argument("--chunk", type=int, default=2000, help="sequences per call (the reference's train chunk)")
    ap.add_argument("--compute_dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--max_tokens", type=int, default=65536,
                    help="bert: packed token rows per call, which the workspace is planned from (2000 captions of about 20 "
                         "word pieces are 40,000 rows); 0 = chunk * 512")
    ap.add_argument("--variant", default=None, choices=list(VARIANTS),
                    help="default: clip_text_b32 for clip, bert_base_uncased for bert")
    return ap


def _tokenize(path, context):
    try:
        import clip
    except ImportError as e:
        raise SystemExit("--captions needs the `clip` package for clip.tokenize (%s); pass --tokens instead" % e)
    with open(path) as f:
        texts = [line.rstrip("\n") for line in f]
    return clip.tokenize(texts, context_length=context)


def _tokenize_bert(path, vocab):
    """(input_ids, attention_mask) of the captions, as the reference's BertTokenizer call makes them
    (networks.py:730-732: padding=True, truncation=True)."""
    if not vocab:
        raise SystemExit("--text_encoder bert --captions needs --vocab (the model's vocab.txt)")
    try:
        from transformers import BertTokenizer
    except ImportError as e:
        raise SystemExit("--captions needs the `transformers` package for BertTokenizer (%s); pass --tokens instead" % e)
    with open(path) as f:
        texts = [line.rstrip("\n") for line in f]
    tok = BertTokenizer(vocab, do_lower_case=True)
    enc = tok(texts, padding=True, truncation=True, max_length=512, return_tensors="pt")
    return enc["input_ids"], enc["attention_mask"]


def _load_bert_tokens(path):
    if path.endswith(".npy"):
        return load_tensor_file(path), None
    ids = load_tensor_file(path, key="tokens")
    try:
        mask = load_tensor_file(path, key="attention_mask")
    except KeyError:
        mask = None
    return ids, mask


def main_bert(args, variant):
    if not args.bert_weights:
        raise SystemExit("--text_encoder bert needs --bert_weights")
    tower = TextTower(variant, max_batch=args.chunk, compute_dtype=args.compute_dtype, max_tokens=args.max_tokens)
    try:
        ids, mask = _load_bert_tokens(args.tokens) if args.tokens else _tokenize_bert(args.captions, args.vocab)
        tower.pack(ids, mask)                       # refuse bad tokens before the weights are read
        tower.load_state_dict_file(args.bert_weights)
        emb = tower.encode(ids, mask).cpu()
    finally:
        tower.close()
    return emb


def main(args):
    if args.chunk < 1:
        raise ValueError("--chunk must be at least 1")
    variant = args.variant or DEFAULT_VARIANT[args.text_encoder]
    if variant not in (BERT_VARIANTS if args.text_encoder == "bert" else CLIP_VARIANTS):
        raise SystemExit("--variant %s is no %s tower" % (variant, args.text_encoder))
    if args.text_encoder == "bert":
        emb = main_bert(args, variant)
        path = write_embed_cache(args, args.file_type, emb, args.embed_dir)
        print("wrote %s: %s float32 (%s, %s)" % (path, tuple(emb.shape), variant, args.compute_dtype))
        return path
    if not args.clip_weights:
        raise SystemExit("--text_encoder clip needs --clip_weights")
    tower = TextTower(variant, max_batch=args.chunk, compute_dtype=args.compute_dtype)
    try:
        ids = load_tensor_file(args.tokens, key="tokens") if args.tokens else _tokenize(args.captions, tower.context)
        ids = tower.check_ids(ids)
        tower.load_state_dict_file(args.clip_weights)
        emb = tower.encode(ids).cpu()
    finally:
        tower.close()
    path = write_embed_cache(args, args.file_type, emb, args.embed_dir)
    print("wrote %s: %s float32 (%s, %s)" % (path, tuple(emb.shape), variant, args.compute_dtype))
    return path


if __name__ == "__main__":
    main(build_parser().parse_args())
