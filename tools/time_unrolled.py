#!/usr/bin/env python3
"""Device-event timing of one whole outer iteration (mdd_unrolled_match) for any engine variant:
    python tools/time_unrolled.py [--variant nf_resnet50] [--n 100] [--K 8] [--size 224] [--dtype bf16] [--steps 5]
                                  [--group8 0 1]
Synthetic expert and targets (networks.synthetic_expert_params / student_move_normalised_targets), random synthetic
set; prints one JSON line with ms per iteration (median of --steps after --warmup) and the workspace size.
--group8 sets mdd_set_group8_kernels (the dedicated grouped 3x3 kernels for 8-channel groups); with both values given the
two settings alternate iteration by iteration in the one process and the line carries `by_group8` with both medians."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="nf_resnet50")
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--d_txt", type=int, default=768)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--keep_steps", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--group8", type=int, nargs="+", choices=[0, 1, 2], default=None)
    a = ap.parse_args()
    import torch
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    from multimodal_dataset_distillation_amd.networks import student_move_normalised_targets, synthetic_expert_params
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(a.n, 3, a.size, a.size, generator=g).to(dev)
    txt = (0.5 * torch.randn(a.n, a.d_txt, generator=g)).to(dev)
    perms = torch.stack([torch.randperm(a.n, generator=g) for _ in range(a.K)]).to(dev)
    lr = torch.tensor([0.1, 0.1], device=dev)
    eng = UnrollEngine(a.variant, batch=a.n, num_queries=a.n, image_size=a.size, d_txt=a.d_txt, syn_steps=a.K,
                       dtype=a.dtype, device=dev, keep_steps=a.keep_steps)
    th = synthetic_expert_params(eng, seed=100, device=dev)
    tgi, tgt = student_move_normalised_targets(eng, th[0], th[1], img, txt, lr, a.K,
                                               torch.Generator(device=dev).manual_seed(200))[:2]
    from multimodal_dataset_distillation_amd import _lib
    lib = _lib.load()
    settings = a.group8 or [None]
    ms = {s: [] for s in settings}
    for it in range(a.warmup + a.steps):
        for s in settings:
            if s is not None:
                lib.mdd_set_group8_kernels(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = eng.unrolled_match(img, txt, lr[0:1], lr[1:2], th[0], th[1], tgi, tgt, perms=perms)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms[s].append(e0.elapsed_time(e1))
    first = settings[0]
    med = statistics.median(ms[first])
    res = dict(variant=a.variant, n=a.n, K=a.K, size=a.size, dtype=a.dtype, keep_steps=a.keep_steps,
               ms_per_iter=med, iters_per_sec=1000.0 / med, ms_all=ms[first],
               workspace_gib=eng.workspace_bytes / 2**30, grand_loss=float(out["grand_loss"]))
    if a.group8:
        res["group8"] = first
        res["by_group8"] = {str(s): dict(ms_per_iter=statistics.median(v), iters_per_sec=1000.0 / statistics.median(v),
                                         ms_all=v) for s, v in ms.items()}
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
