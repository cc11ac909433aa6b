"""Writes tests/golden/clip_text_block_small.npz: one CAUSAL CLIP transformer block run by the REFERENCE's own code.

Build-machine only (it needs a checkout of the reference; nothing of the reference is copied into the repository -- the
fixture holds numeric arrays and parameter names).

    python tools/gen_clip_text_golden.py --reference /path/to/reference

The reference's `model.py` is imported as it is and its `ResidualAttentionBlock(64, 2, attn_mask=causal)` -- the block of
CLIP's text transformer: nn.MultiheadAttention under the additive mask that holds -inf above the diagonal, LayerNorm in
fp32 with eps 1e-5, QuickGELU -- is run in fp32 on 33 tokens x 3 sequences with seeded parameters (perturbed LayerNorm
gains, every bias non-zero).  Stored: the input `x` as [sequences, tokens, width] (the reference's block takes [tokens,
sequences, width]: transposed here, once), `param.<name>` for every parameter under the block's own names, the output
`y`.  tests/test_clip_text_cpu.py runs tests/clip_text_ref.py's block in float64 on the same numbers.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEADS, TOKENS, SEQS = 64, 2, 33, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MDD_REFERENCE_DIR", ""), help="checkout of the reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "clip_text_block_small.npz"))
    args = ap.parse_args()
    if not os.path.isfile(os.path.join(args.reference, "model.py")):
        raise SystemExit("--reference must name a directory that holds the reference's model.py")
    sys.path.insert(0, args.reference)
    import model as ref_model   # the reference's own file

    torch.manual_seed(30)
    mask = torch.full((TOKENS, TOKENS), float("-inf")).triu_(1)          # additive: -inf above the diagonal, 0 elsewhere
    blk = ref_model.ResidualAttentionBlock(WIDTH, HEADS, attn_mask=mask).float()
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name in ("ln_1.weight", "ln_2.weight"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):          # every bias, the attention's zero-initialised ones included
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    x = torch.randn(SEQS, TOKENS, WIDTH, generator=g)
    with torch.no_grad():
        y = blk(x.transpose(0, 1).contiguous())                           # [tokens, sequences, width]
    names = [n for n, _ in blk.named_parameters()]
    out = {"x": x.numpy(), "y": y.transpose(0, 1).contiguous().numpy(), "names": np.array(names), "heads": np.array(HEADS)}
    for n, p in blk.named_parameters():
        out["param." + n] = p.detach().numpy()
    np.savez(args.out, **out)
    print("wrote %s (%d bytes): %s" % (args.out, os.path.getsize(args.out), ", ".join(names)))


if __name__ == "__main__":
    main()
