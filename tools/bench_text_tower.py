"""Times the frozen CLIP text tower: HIP events around `mdd_text_tower_encode` (one library call per timed interval, ids
already on the device and checked), `--batch` sequences per call, `--calls` timed calls after `--warmup` untimed ones.

    python tools/bench_text_tower.py [--variant clip_text_b32] [--compute_dtype bf16] [--batch 2000] [--out FILE.json]

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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from multimodal_dataset_distillation_amd.text_tower import TextTower
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
               mmac_per_token=round(mmac_token, 3), tflops_per_s=round(2 * mmac_token * 1e6 * tokens / (mean_ms * 1e-3) / 1e12, 1),
               workspace_bytes=int(tw.workspace_bytes), device=torch.cuda.get_device_name(0))
    tw.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
