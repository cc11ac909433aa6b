"""TEST INFRASTRUCTURE ONLY -- float64-capable PyTorch restatement of the CLIP image tower (`--image_encoder clip`).

What it restates
----------------
OpenAI CLIP's published `VisionTransformer` (clip/model.py), ViT-B/32 as `clip.load("ViT-B/32")` builds it and as the
reference reaches it through `encode_image` (networks.py:659-662).  With g = image_size / patch:

    x = conv1(img)                              Conv2d(3, D, kernel = P, stride = P, bias = False) -> [N, g*g, D], row-major
    x = cat(class_embedding, x) + positional_embedding          [N, T = 1 + g*g, D]
    x = ln_pre(x)
    for each block:
        x = x + out_proj(attention(in_proj(ln_1(x))))           heads H, head dim D/H, scale (D/H)^-0.5
        x = x + c_proj(QuickGELU(c_fc(ln_2(x))))                hidden 4 D, QuickGELU(v) = v * sigmoid(1.702 v)
    y = ln_post(x[:, 0]) @ proj                                 proj [D, out], no bias; eps = 1e-5 in every LayerNorm

Pinning: the BLOCK is pinned to the reference's own `model.py` (`ResidualAttentionBlock`, importable on the build
machine) through tests/golden/clip_block_small.npz (tools/gen_clip_golden.py; tests/test_clip_vit_cpu.py).  The tower around
it is not in the reference tree (the `clip` package is absent) and is PARITY UNPINNED like every other encoder: it follows
the published source; structural anchor 87,849,216 parameters for ViT-B/32 at 224.

Parameter order (theta is ONE flat vector in `named_modules() x named_parameters(recurse=False)` order, reference
reparam_module.py:28-39): the tower's own parameters first (class_embedding, positional_embedding, proj), then conv1,
ln_pre, transformer.resblocks.i.{attn (in_proj_weight, in_proj_bias, out_proj), ln_1, mlp.c_fc, mlp.c_proj, ln_2},
ln_post; every name under `model.visual.` because the reference's `ImageEncoder.model` is the whole CLIP object.  Only
the visual tower is restated (and is the student's theta): CLIP's text tower receives no gradient in either stage.
"""
from dataclasses import dataclass

import torch
import torch.nn as nn


@dataclass
class ClipCfg:
    img_size: int = 224
    patch: int = 32
    dim: int = 768
    depth: int = 12
    heads: int = 12
    out: int = 512
    eps: float = 1e-5


VARIANTS = {
    "clip_vit_b32": ClipCfg(),                                                          # clip.load("ViT-B/32").visual
    "clip_vit_micro": ClipCfg(img_size=32, patch=8, dim=64, depth=2, heads=2, out=24),   # MLP 256 wide: fused epilogues
    "clip_vit_nano": ClipCfg(img_size=32, patch=8, dim=16, depth=2, heads=2, out=8),     # MLP 64 wide: chunk kernels
}


class SelfAttention(nn.Module):
    """Self-attention with nn.MultiheadAttention's parameters (in_proj_weight [3D, D] = q | k | v rows, in_proj_bias,
    out_proj) on [N, T, D], written out so that torch.func can differentiate it twice in any dtype."""

    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        self.out_proj = nn.Linear(dim, dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)

    def forward(self, x):
        n, t, d = x.shape
        hd = d // self.heads
        qkv = x @ self.in_proj_weight.t() + self.in_proj_bias
        q, k, v = (z.reshape(n, t, self.heads, hd).transpose(1, 2) for z in qkv.split(d, dim=-1))   # [N, H, T, hd]
        p = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
        return self.out_proj((p @ v).transpose(1, 2).reshape(n, t, d))


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.c_fc = nn.Linear(dim, 4 * dim)
        self.gelu = QuickGELU()
        self.c_proj = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.c_proj(self.gelu(self.c_fc(x)))


class Block(nn.Module):
    def __init__(self, dim, heads, eps=1e-5):
        super().__init__()
        self.attn = SelfAttention(dim, heads)
        self.ln_1 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim)
        self.ln_2 = nn.LayerNorm(dim, eps=eps)

    def forward(self, x):
        x = x + self.attn(self.ln_1(x))
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, eps):
        super().__init__()
        self.resblocks = nn.Sequential(*[Block(dim, heads, eps) for _ in range(depth)])

    def forward(self, x):
        return self.resblocks(x)


class VisionTransformer(nn.Module):
    def __init__(self, cfg: ClipCfg, img_size=None):
        super().__init__()
        size = img_size or cfg.img_size
        assert size % cfg.patch == 0
        self.cfg = cfg
        self.num_tokens = 1 + (size // cfg.patch) ** 2
        scale = cfg.dim ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(cfg.dim))
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.num_tokens, cfg.dim))
        self.proj = nn.Parameter(scale * torch.randn(cfg.dim, cfg.out))
        self.conv1 = nn.Conv2d(3, cfg.dim, kernel_size=cfg.patch, stride=cfg.patch, bias=False)
        self.ln_pre = nn.LayerNorm(cfg.dim, eps=cfg.eps)
        self.transformer = Transformer(cfg.dim, cfg.depth, cfg.heads, cfg.eps)
        self.ln_post = nn.LayerNorm(cfg.dim, eps=cfg.eps)

    def forward(self, x):
        x = self.conv1(x).flatten(2).transpose(1, 2)                      # [N, g*g, D], row-major over the patch grid
        cls = self.class_embedding.expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding
        x = self.transformer(self.ln_pre(x))
        return self.ln_post(x[:, 0]) @ self.proj


class ClipShell(nn.Module):
    """What the reference's ImageEncoder.model is for `clip`: an object with `.visual` and `encode_image`."""

    def __init__(self, cfg, img_size=None):
        super().__init__()
        self.visual = VisionTransformer(cfg, img_size)
        self.num_features = cfg.out

    def encode_image(self, x):
        return self.visual(x)


class ImageEncoder(nn.Module):
    """Same wrapper shape as oracle/vit_ref.ImageEncoder (reference networks.py:648-682: `self.model`)."""

    def __init__(self, variant="clip_vit_b32", img_size=None):
        super().__init__()
        self.model = ClipShell(VARIANTS[variant], img_size)

    def forward(self, x):
        return self.model.encode_image(x)


def randomize_like_trained(module: nn.Module, seed: int):
    """Break the symmetric default init (unit LayerNorm gains, zero LayerNorm / attention biases) so that every
    parameter carries a gradient of ordinary size in the parity tests."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if ("ln_" in name) and leaf == "weight":
                p.add_((0.1 * torch.randn(p.shape, generator=g)).to(p.dtype))
            elif leaf in ("bias", "in_proj_bias"):
                p.add_((0.02 * torch.randn(p.shape, generator=g)).to(p.dtype))
            elif leaf == "class_embedding":
                p.add_((0.02 * torch.randn(p.shape, generator=g)).to(p.dtype))
