"""Writes tests/golden/clip_block_small.npz: one CLIP transformer block run by the REFERENCE's own code.

Build-machine only (it needs a checkout of the reference; nothing of the reference is copied into the repository -- the
fixture holds numeric arrays and parameter names).

    python tools/gen_clip_golden.py --reference /path/to/reference

The reference's `model.py` is imported as it is and its `ResidualAttentionBlock(64, 2)` (nn.MultiheadAttention,
LayerNorm in fp32 with eps 1e-5, QuickGELU) is run in fp32 on 17 tokens x 3 images with seeded parameters (perturbed
LayerNorm gains, every bias non-zero) and a seeded cotangent.  Stored: the input `x` and cotangent `w` as [images,
tokens, width] (the reference's block takes [tokens, images, width]: transposed here, once), `param.<name>` for every
parameter under the block's own names, the output `y`, `grad.x` and `grad.<name>`.
tests/test_clip_vit_cpu.py runs tests/clip_vit_ref.py's block in float64 on the same numbers.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEADS, TOKENS, IMAGES = 64, 2, 17, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MDD_REFERENCE_DIR", ""), help="checkout of the reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "clip_block_small.npz"))
    args = ap.parse_args()
    if not os.path.isfile(os.path.join(args.reference, "model.py")):
        raise SystemExit("--reference must name a directory that holds the reference's model.py")
    sys.path.insert(0, args.reference)
    import model as ref_model   # the reference's own file

    torch.manual_seed(20)
    blk = ref_model.ResidualAttentionBlock(WIDTH, HEADS).float()
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name in ("ln_1.weight", "ln_2.weight"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):          # every bias, the attention's zero-initialised ones included
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    x = torch.randn(IMAGES, TOKENS, WIDTH, generator=g)
    w = torch.randn(IMAGES, TOKENS, WIDTH, generator=g)
    xin = x.transpose(0, 1).contiguous().requires_grad_(True)           # [tokens, images, width]
    y = blk(xin)
    names = [n for n, _ in blk.named_parameters()]
    grads = torch.autograd.grad(y, [xin] + [p for _, p in blk.named_parameters()], w.transpose(0, 1).contiguous())
    out = {"x": x.numpy(), "w": w.numpy(), "y": y.detach().transpose(0, 1).contiguous().numpy(),
           "grad.x": grads[0].transpose(0, 1).contiguous().numpy(), "names": np.array(names),
           "heads": np.array(HEADS)}
    for (n, p), gp in zip(blk.named_parameters(), grads[1:]):
        out["param." + n] = p.detach().numpy()
        out["grad." + n] = gp.numpy()
    np.savez(args.out, **out)
    print("wrote %s (%d bytes): %s" % (args.out, os.path.getsize(args.out), ", ".join(names)))


if __name__ == "__main__":
    main()
