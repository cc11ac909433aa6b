"""Writes tests/golden/bert_layer_small.npz: one BERT encoder layer run by `transformers`' own code.

Build-machine only (it needs the `transformers` package, the one the reference calls; nothing of it is copied into the
repository -- the fixture holds numeric arrays and parameter names).  No weights are fetched: the layer is built from a
`BertConfig` and seeded here.

    python tools/gen_bert_golden.py

`transformers.models.bert.modeling_bert.BertLayer` -- hidden 64, 2 heads, intermediate 256, eps 1e-12, exact GELU, eval
mode -- is run on the CPU in fp32 on 3 sequences padded to 33 tokens, of lengths 33, 20 and 1, under the additive key mask
BertModel builds from an attention_mask (0 over a sequence, the dtype's most negative number over its padding).  Stored:
the input `x` [3, 33, 64], `param.<name>` for every parameter under the layer's own names, the output `y` (its rows beyond
a sequence's length are the layer's values for padded queries: nothing reads them), `names`, `heads`, `lens`.
tests/test_bert_cpu.py runs tests/bert_ref.py's layer in float64 on the same numbers.
"""
import argparse
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEADS, INTER, TOKENS = 64, 2, 256, 33
LENS = [33, 20, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bert_layer_small.npz"))
    args = ap.parse_args()
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertLayer

    torch.manual_seed(40)
    cfg = BertConfig(hidden_size=WIDTH, num_attention_heads=HEADS, intermediate_size=INTER, num_hidden_layers=1,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    try:
        cfg._attn_implementation = "eager"          # the plain softmax(QK^T + mask)V path
    except Exception:
        pass
    layer = BertLayer(cfg).float().eval()
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if p.dim() == 2:
                p.copy_(p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g))     # scores with a spread of about one
            elif "LayerNorm" in name and leaf == "weight":
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))                    # every bias non-zero
    x = torch.randn(len(LENS), TOKENS, WIDTH, generator=g)
    keep = torch.arange(TOKENS)[None, :] < torch.tensor(LENS)[:, None]
    mask = torch.zeros(len(LENS), 1, 1, TOKENS).masked_fill_(~keep[:, None, None, :], torch.finfo(torch.float32).min)
    with torch.no_grad():
        y = layer(x, attention_mask=mask)
    if isinstance(y, (tuple, list)):
        y = y[0]
    names = [n for n, _ in layer.named_parameters()]
    out = {"x": x.numpy(), "y": y.numpy(), "names": np.array(names), "heads": np.array(HEADS), "lens": np.array(LENS)}
    for n, p in layer.named_parameters():
        out["param." + n] = p.detach().numpy()
    np.savez(args.out, **out)
    print("wrote %s (%d bytes): %s" % (args.out, os.path.getsize(args.out), ", ".join(names)))


if __name__ == "__main__":
    main()
