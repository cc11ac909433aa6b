"""Times the frozen text towers: HIP events around `mdd_text_tower_encode` / `mdd_text_tower_encode_varlen` (one library
call per timed interval, ids already on the device and checked), `--batch` sequences per call, `--calls` timed calls after
`--warmup` untimed ones.

    python tools/bench_text_tower.py [--variant clip_text_b32] [--compute_dtype bf16] [--batch 2000] [--out FILE.json]
    python tools/bench_text_tower.py --variant bert_base_uncased --lengths caption|fixed:L [--batch 2000]

BERT variants run over packed tokens.  `--lengths caption` draws caption-like lengths (seeded): 2 + a whole number from a
log-normal with median 16 and sigma 0.45, cut to [3, 80] -- [CLS] and [SEP] included, most captions around 18 word pieces,
a tail to about 80, the shape of Flickr30k / COCO captions under BERT's tokenizer.  `--lengths fixed:L` gives every
sequence L tokens: with L the longest length of the caption draw (printed as `max_len`), that is the work the
reference's padding does.  Per token the multiply-accumulates are layers * 12 width^2 for the linears plus 2 * len * width
per layer for the two attention products; reported: captions/s, tokens/s and TFLOP/s.

Prints (and writes) one JSON object: captions/s, the achieved TFLOP/s against the multiply-accumulates of the blocks
(per token and layer 12 width^2 for the four linears plus (context + 1) width for the two causal attention products:
38.2 MMAC per token for ViT-B/32's text tower), and the workspace size.  The weights are random; the ids carry an
end-of-text token at a random position with zero padding behind it, as clip.tokenize writes them.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="clip_text_b32")
    ap.add_argument("--compute_dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lengths", default="caption", help="BERT variants: caption | fixed:L")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from multimodal_dataset_distillation_amd.text_tower import BERT_VARIANTS, TextTower
    if args.variant in BERT_VARIANTS:
        return bench_bert(args)
    tw = TextTower(args.variant, max_batch=args.batch, compute_dtype=args.compute_dtype)
    g = torch.Generator().manual_seed(0)
    theta = torch.empty(tw.param_numel)
    width = layers = 0
    for name, shape, off in tw.param_table():
        n = 1
        for s in shape:
            n *= s
        if ".ln_" in name and name.endswith("weight"):
            t = torch.ones(n)
        elif name.endswith("bias"):
            t = 0.02 * torch.randn(n, generator=g)
        else:
            t = shape[-1] ** -0.5 * torch.randn(n, generator=g) if len(shape) == 2 else torch.zeros(n)
        theta[off:off + n] = t
        if name == "model.positional_embedding":
            width = shape[1]
        if name.endswith("attn.in_proj_weight"):
            layers += 1
    tw.load_flat(theta)
    ids = torch.randint(1, tw.vocab - 2, (args.batch, tw.context), generator=g)
    eot = torch.randint(1, tw.context, (args.batch,), generator=g)
    pos = torch.arange(tw.context)[None, :]
    ids = torch.where(pos < eot[:, None], ids, torch.zeros_like(ids))
    ids[torch.arange(args.batch), eot] = tw.vocab - 1
    import ctypes as C
    from multimodal_dataset_distillation_amd._lib import check
    ids = tw.check_ids(ids).to("cuda").contiguous()
    y = torch.empty(args.batch, tw.feature_dim, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def encode():
        check(tw.lib.mdd_text_tower_encode(tw.h, C.c_void_p(ids.data_ptr()), args.batch, C.c_void_p(y.data_ptr()), stream))
    for _ in range(args.warmup):
        encode()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    for a, b in ev:
        a.record()
        encode()
        b.record()
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    mean_ms = sum(ms) / len(ms)
    mmac_token = layers * (12 * width * width + (tw.context + 1) * width) / 1e6
    tokens = args.batch * tw.context
    res = dict(variant=args.variant, compute_dtype=args.compute_dtype, sequences_per_call=args.batch, calls=args.calls,
               warmup=args.warmup, ms_per_call_mean=round(mean_ms, 3), ms_per_call_min=round(ms[0], 3),
               ms_per_call_max=round(ms[-1], 3), captions_per_s=round(args.batch / (mean_ms * 1e-3), 1),
               tokens_per_s=round(tokens / (mean_ms * 1e-3), 1), mmac_per_token=round(mmac_token, 3), tflops_per_s=round(2 * mmac_token * 1e6 * tokens / (mean_ms * 1e-3) / 1e12, 1),
               workspace_bytes=int(tw.workspace_bytes), device=torch.cuda.get_device_name(0))
    tw.close()
    emit(res, args.out)


def emit(res, out):
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def caption_lengths(n, positions, seed=0):
    """Seeded caption-like lengths: 2 ([CLS], [SEP]) + round(lognormal(median 16, sigma 0.45)), cut to [3, min(80, positions)]."""
    g = torch.Generator().manual_seed(seed)
    body = torch.exp(torch.log(torch.tensor(16.0)) + 0.45 * torch.randn(n, generator=g)).round().long()
    return (2 + body).clamp_(3, min(80, positions)).tolist()


def bench_bert(args):
    import ctypes as C
    from multimodal_dataset_distillation_amd._lib import check
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    probe = TextTower(args.variant, max_batch=1, compute_dtype=args.compute_dtype, bind=False)
    positions, vocab = probe.context, probe.vocab
    probe.close()
    if args.lengths == "caption":
        lens = caption_lengths(args.batch, positions)
    elif args.lengths.startswith("fixed:"):
        lens = [int(args.lengths.split(":")[1])] * args.batch
        if not 1 <= lens[0] <= positions:
            raise SystemExit("fixed:L needs 1 <= L <= %d" % positions)
    else:
        raise SystemExit("--lengths is caption or fixed:L")
    total, max_len = sum(lens), max(lens)
    tw = TextTower(args.variant, max_batch=args.batch, compute_dtype=args.compute_dtype, max_tokens=total)
    g = torch.Generator().manual_seed(0)
    theta = torch.empty(tw.param_numel)
    width = layers = 0
    for name, shape, off in tw.param_table():
        n = 1
        for s in shape:
            n *= s
        if "LayerNorm" in name and name.endswith("weight"):
            t = torch.ones(n)
        elif name.endswith("bias"):
            t = 0.02 * torch.randn(n, generator=g)
        elif "embeddings" in name:
            t = 0.02 * torch.randn(n, generator=g)
        else:
            t = shape[-1] ** -0.5 * torch.randn(n, generator=g)
        theta[off:off + n] = t
        if name == "embeddings.word_embeddings.weight":
            width = shape[1]
        if name.endswith("attention.self.query.weight"):
            layers += 1
    tw.load_flat(theta)
    ids = torch.randint(1, vocab, (total,), generator=g, dtype=torch.int32).to("cuda")
    cu = torch.tensor([0] + lens).cumsum(0).to(torch.int32).to("cuda")
    y = torch.empty(args.batch, tw.feature_dim, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def encode():
        check(tw.lib.mdd_text_tower_encode_varlen(tw.h, C.c_void_p(ids.data_ptr()), C.c_void_p(cu.data_ptr()), args.batch,
                                                  total, max_len, C.c_void_p(y.data_ptr()), stream))
    for _ in range(args.warmup):
        encode()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    for a, b in ev:
        a.record()
        encode()
        b.record()
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    mean_ms = sum(ms) / len(ms)
    macs = layers * (12 * width * width * total + 2 * width * sum(l * l for l in lens))
    res = dict(variant=args.variant, compute_dtype=args.compute_dtype, lengths=args.lengths, sequences_per_call=args.batch,
               tokens_per_call=total, max_len=max_len, mean_len=round(total / args.batch, 2), calls=args.calls,
               warmup=args.warmup, ms_per_call_mean=round(mean_ms, 3), ms_per_call_min=round(ms[0], 3),
               ms_per_call_max=round(ms[-1], 3), captions_per_s=round(args.batch / (mean_ms * 1e-3), 1),
               tokens_per_s=round(total / (mean_ms * 1e-3), 1), mmac_per_token=round(macs / total / 1e6, 3),
               tflops_per_s=round(2 * macs / (mean_ms * 1e-3) / 1e12, 1), workspace_bytes=int(tw.workspace_bytes),
               device=torch.cuda.get_device_name(0))
    tw.close()
    emit(res, args.out)


if __name__ == "__main__":
    main()
