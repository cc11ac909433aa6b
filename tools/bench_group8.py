#!/usr/bin/env python3
"""Op-level timing of NF-RegNet-B1's grouped 3x3 convolutions (8 channels per group) in bf16 at N = 100: the dedicated
kernel of csrc/conv_g8.hip against the general implicit-GEMM kernels (mdd_set_group8_kernels(0)), in ONE process,
alternating, after warm-up, device-event times, median of --reps.

    python tools/bench_group8.py [--n 100] [--reps 25] [--out profiles/nf_regnet_b1_group8_bench.json]

For every real conv2 geometry of the network (groups, input side, stride) and the passes that have a dedicated kernel
(forward, data gradient; mdd_set_group8_kernels(2) routes every geometry to it) it records both medians, the run-to-run
spread of each (max - min of the timed repetitions), the kernel's algorithmic bytes (every operand read once, the
result written once) over its time as a share of 8 TB/s, and `faster`: whether the dedicated kernel won by more than the larger spread -- the condition under
which csrc/conv_g8.hip's g8_routes() may send that geometry / pass to it.
The weight gradient is not timed: it has no dedicated kernel (every geometry runs k_conv_wgrad).  One was written, measured
1.6 to 8.6 times slower and removed; profiles/nf_regnet_b1_group8_wgrad_attempt.json keeps that measurement as a record and
cannot be regenerated from this tree."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (groups, input side, stride): conv2 of the blocks 0.0 | 0.1 | 1.0 | 1.1-1.3 | 2.0 | 2.1-2.6 | 3.0 | 3.1-3.6
GEOMETRIES = [(5, 112, 2), (11, 56, 1), (11, 56, 2), (23, 28, 1), (23, 28, 2), (45, 14, 1), (45, 14, 2), (92, 7, 1)]
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from multimodal_dataset_distillation_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    bf = torch.bfloat16
    rows = []
    prev = lib.mdd_set_group8_kernels(2)
    for groups, side, stride in GEOMETRIES:
        ch, n = groups * 8, a.n
        ho = (side + 2 - 3) // stride + 1
        x = torch.randn(n, side, side, ch, device=dev).to(bf)
        dy = torch.randn(n, ho, ho, ch, device=dev).to(bf)
        wf = (torch.randn(ch, 9, 8, device=dev) / 72 ** 0.5).to(bf)
        wt = (torch.randn(groups, 8, 9, 8, device=dev) / 72 ** 0.5).to(bf)
        bias = torch.randn(ch, device=dev)
        yo, dxo = torch.empty_like(dy), torch.empty_like(x)
        ein, eout, ew = x.numel() * 2, dy.numel() * 2, wf.numel() * 2
        passes = {
            "forward": (lambda: lib.mdd_op_conv2d(1, 0, n, side, side, ch, ch, 3, stride, 1, groups, P(x), P(wf), P(bias),
                                                  P(yo), st), ein + eout + ew),
            "data_gradient": (lambda: lib.mdd_op_conv2d(1, 1, n, side, side, ch, ch, 3, stride, 1, groups, P(dy), P(wt),
                                                        None, P(dxo), st), ein + eout + ew),
        }
        for name, (fn, nbytes) in passes.items():
            ms = {2: [], 0: []}
            for it in range(a.warmup + a.reps):
                for on in (2, 0):
                    lib.mdd_set_group8_kernels(on)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _lib.check(fn())
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        ms[on].append(e0.elapsed_time(e1))
            med = {on: statistics.median(v) for on, v in ms.items()}
            spread = {on: max(v) - min(v) for on, v in ms.items()}
            row = dict(groups=groups, side=side, stride=stride, n=n, pass_=name, bytes=nbytes,
                       dedicated_ms=med[2], general_ms=med[0], dedicated_spread_ms=spread[2], general_spread_ms=spread[0],
                       dedicated_hbm_share=nbytes / (med[2] * 1e-3) / HBM_BYTES_PER_S,
                       general_hbm_share=nbytes / (med[0] * 1e-3) / HBM_BYTES_PER_S,
                       faster=bool(med[0] - med[2] > max(spread.values())))
            rows.append(row)
            print(json.dumps(row), flush=True)
    lib.mdd_set_group8_kernels(prev)
    res = dict(tool="tools/bench_group8.py", reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
