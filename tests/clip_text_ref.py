"""TEST INFRASTRUCTURE ONLY -- float64-capable PyTorch restatement of CLIP's text tower (`--text_encoder clip`).

What it restates
----------------
OpenAI CLIP's published `encode_text` (clip/model.py), as `clip.load("ViT-B/32")` builds it and as the reference reaches
it through `TextEncoder.forward` (networks.py:723-726) to write the caption caches (distill.py:107-144):

    x = token_embedding(ids) + positional_embedding                 [N, T = 77, D]
    for each block (the image tower's block, tests/clip_vit_ref.py, under an additive attention mask that holds -inf
    above the diagonal: position t attends to positions 0 .. t):
        x = x + out_proj(attention(in_proj(ln_1(x)), mask))
        x = x + c_proj(QuickGELU(c_fc(ln_2(x))))
    x = ln_final(x)
    y = x[arange(N), ids.argmax(-1)] @ text_projection              the end-of-text token has the largest id

Pinning: the BLOCK is pinned to the reference's own `model.py` (`ResidualAttentionBlock(64, 2, attn_mask=causal)`)
through tests/golden/clip_text_block_small.npz (tools/gen_clip_text_golden.py; tests/test_clip_text_cpu.py).  The tower
around it is not in the reference tree (the `clip` package is absent) and follows the published source; structural anchor
63,428,096 parameters = 151,277,313 (whole CLIP ViT-B/32) - 87,849,216 (visual tower) - 1 (logit_scale).

Parameter names are the `clip` package's (`CLIP.named_parameters()`, the text tower's entries), under `model.` as the image
tower's are: positional_embedding, text_projection, transformer.resblocks.i.{attn.in_proj_weight, attn.in_proj_bias,
attn.out_proj, ln_1, mlp.c_fc, mlp.c_proj, ln_2}, token_embedding.weight, ln_final.
"""
from dataclasses import dataclass

import torch
import torch.nn as nn

from clip_vit_ref import Block, SelfAttention, randomize_like_trained  # noqa: F401  (re-exported for the tests)


@dataclass
class TextCfg:
    vocab: int = 49408
    ctx: int = 77
    width: int = 512
    heads: int = 8
    layers: int = 12
    embed: int = 512
    eps: float = 1e-5


VARIANTS = {
    "clip_text_b32": TextCfg(),                                                               # clip.load("ViT-B/32")
    "clip_text_micro": TextCfg(vocab=512, ctx=77, width=128, heads=2, layers=2, embed=24),     # the real context
    "clip_text_nano": TextCfg(vocab=64, ctx=33, width=64, heads=1, layers=2, embed=8),         # one row past a tile, one head
}


class CausalSelfAttention(SelfAttention):
    """tests/clip_vit_ref.SelfAttention with nn.MultiheadAttention's additive attn_mask: -inf above the diagonal."""

    def forward(self, x):
        n, t, d = x.shape
        hd = d // self.heads
        qkv = x @ self.in_proj_weight.t() + self.in_proj_bias
        q, k, v = (z.reshape(n, t, self.heads, hd).transpose(1, 2) for z in qkv.split(d, dim=-1))   # [N, H, T, hd]
        mask = torch.full((t, t), float("-inf"), dtype=x.dtype, device=x.device).triu_(1)
        p = ((q * hd ** -0.5) @ k.transpose(-2, -1) + mask).softmax(dim=-1)
        return self.out_proj((p @ v).transpose(1, 2).reshape(n, t, d))


class CausalBlock(Block):
    def __init__(self, dim, heads, eps=1e-5):
        super().__init__(dim, heads, eps)
        self.attn = CausalSelfAttention(dim, heads)      # same parameters, same registration slot


class TextTransformer(nn.Module):
    def __init__(self, dim, layers, heads, eps):
        super().__init__()
        self.resblocks = nn.Sequential(*[CausalBlock(dim, heads, eps) for _ in range(layers)])

    def forward(self, x):
        return self.resblocks(x)


class ClipText(nn.Module):
    """The text half of clip/model.py's CLIP, parameters registered in CLIP's order."""

    def __init__(self, cfg: TextCfg):
        super().__init__()
        self.cfg = cfg
        self.transformer = TextTransformer(cfg.width, cfg.layers, cfg.heads, cfg.eps)
        self.token_embedding = nn.Embedding(cfg.vocab, cfg.width)
        self.positional_embedding = nn.Parameter(torch.empty(cfg.ctx, cfg.width))
        self.ln_final = nn.LayerNorm(cfg.width, eps=cfg.eps)
        self.text_projection = nn.Parameter(torch.empty(cfg.width, cfg.embed))
        # CLIP.initialize_parameters
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std = cfg.width ** -0.5 * (2 * cfg.layers) ** -0.5
        attn_std, fc_std = cfg.width ** -0.5, (2 * cfg.width) ** -0.5
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=cfg.width ** -0.5)

    def hidden(self, ids):
        """ln_final of every position: [N, T, D]."""
        x = self.token_embedding(ids) + self.positional_embedding
        return self.ln_final(self.transformer(x))

    def encode_text(self, ids):
        x = self.hidden(ids)
        return x[torch.arange(x.shape[0]), ids.argmax(dim=-1)] @ self.text_projection


class TextEncoder(nn.Module):
    """`self.model` as in the reference's TextEncoder (networks.py:701): parameter names start with `model.`."""

    def __init__(self, variant="clip_text_b32"):
        super().__init__()
        self.model = ClipText(VARIANTS[variant])

    def forward(self, ids):
        return self.model.encode_text(ids)


def named_shapes(module):
    return [(n, tuple(p.shape)) for n, p in module.named_parameters()]
