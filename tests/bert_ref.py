"""TEST INFRASTRUCTURE ONLY -- float64-capable PyTorch restatement of BERT's encoder (`--text_encoder bert`).

What it restates
----------------
`transformers`' `BertModel("bert-base-uncased")` as the reference's `TextEncoder.forward` calls it (networks.py:703-735):
`model(input_ids, attention_mask).last_hidden_state[:, 0]`, no token_type_ids (every token is of type 0), eval mode (no
dropout), the pooler unused:

    x = LayerNorm(word_embeddings[ids] + position_embeddings[0 .. L) + token_type_embeddings[0])
    per layer (post-LN):
        a = softmax(q k^T / sqrt(64) + key mask) v          query / key / value are three linears; the additive key mask
                                                            removes the padded positions of each sequence
        x = LayerNorm(x + dense(a))
        x = LayerNorm(x + dense(GELU(dense(x))))            exact (erf) GELU, 4 x width
    y = x[:, 0]                                             the [CLS] row

LayerNorm eps is 1e-12.  Two forwards compute the same numbers: `forward(ids, attention_mask)` on the padded batch, as
the reference runs it, and `forward_packed(ids_packed, lens)` on the tokens alone -- sum(len) rows, the attention per
sequence -- which is how the library runs it.

Pinning: the LAYER is pinned to `transformers.models.bert.modeling_bert.BertLayer` -- the class the reference calls --
through tests/golden/bert_layer_small.npz (tools/gen_bert_golden.py; tests/test_bert_cpu.py), and the whole model to a
random-weight `BertModel` where the package is installed.  Structural anchor: 108,891,648 parameters = 109,482,240
(BertModel of bert-base-uncased) - 590,592 (its pooler).

Parameter names are BertModel's own, bare: embeddings.{word,position,token_type}_embeddings.weight, embeddings.LayerNorm,
encoder.layer.i.{attention.self.{query,key,value}, attention.output.{dense,LayerNorm}, intermediate.dense,
output.{dense,LayerNorm}}.
"""
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class BertCfg:
    vocab: int = 30522
    positions: int = 512
    width: int = 768
    heads: int = 12
    layers: int = 12
    intermediate: int = 3072
    type_vocab: int = 2
    eps: float = 1e-12


VARIANTS = {
    "bert_base_uncased": BertCfg(),                                                          # transformers BertConfig()
    "bert_micro": BertCfg(vocab=512, positions=512, width=128, heads=2, layers=2, intermediate=512),
    "bert_nano": BertCfg(vocab=64, positions=40, width=64, heads=1, layers=2, intermediate=256),
}


class SelfAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.query, self.key, self.value = nn.Linear(dim, dim), nn.Linear(dim, dim), nn.Linear(dim, dim)

    def forward(self, x, key_mask=None):
        """x [..., T, D]; key_mask additive [..., T] over the keys (0 or -inf) or None."""
        *lead, t, d = x.shape
        hd = d // self.heads
        q, k, v = (f(x).reshape(*lead, t, self.heads, hd).transpose(-3, -2) for f in (self.query, self.key, self.value))
        s = q @ k.transpose(-2, -1) * hd ** -0.5                                     # [..., H, T, T]
        if key_mask is not None:
            s = s + key_mask[..., None, None, :]
        return (s.softmax(dim=-1) @ v).transpose(-3, -2).reshape(*lead, t, d)


class SelfOutput(nn.Module):
    def __init__(self, cin, dim, eps):
        super().__init__()
        self.dense = nn.Linear(cin, dim)
        self.LayerNorm = nn.LayerNorm(dim, eps=eps)

    def forward(self, h, x):
        return self.LayerNorm(x + self.dense(h))


class Attention(nn.Module):
    def __init__(self, dim, heads, eps):
        super().__init__()
        self.add_module("self", SelfAttention(dim, heads))
        self.output = SelfOutput(dim, dim, eps)

    def forward(self, x, key_mask=None):
        return self.output(getattr(self, "self")(x, key_mask), x)


class Intermediate(nn.Module):
    def __init__(self, dim, inter):
        super().__init__()
        self.dense = nn.Linear(dim, inter)

    def forward(self, x):
        return F.gelu(self.dense(x))                       # exact (erf)


class BertLayer(nn.Module):
    """transformers' BertLayer, parameters registered in its order."""

    def __init__(self, dim, heads, inter, eps=1e-12):
        super().__init__()
        self.attention = Attention(dim, heads, eps)
        self.intermediate = Intermediate(dim, inter)
        self.output = SelfOutput(inter, dim, eps)

    def forward(self, x, key_mask=None):
        x = self.attention(x, key_mask)
        return self.output(self.intermediate(x), x)

    # packed: x [total, D]; the linears over every row, the attention per sequence
    def forward_packed(self, x, lens):
        att = getattr(self.attention, "self")
        a = torch.cat([att(s) for s in x.split(list(lens), dim=0)], dim=0)
        x = self.attention.output(a, x)
        return self.output(self.intermediate(x), x)


class Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = nn.Embedding(cfg.vocab, cfg.width)
        self.position_embeddings = nn.Embedding(cfg.positions, cfg.width)
        self.token_type_embeddings = nn.Embedding(cfg.type_vocab, cfg.width)
        self.LayerNorm = nn.LayerNorm(cfg.width, eps=cfg.eps)

    def forward(self, ids, positions):
        return self.LayerNorm(self.word_embeddings(ids) + self.position_embeddings(positions)
                              + self.token_type_embeddings.weight[0])


class Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(cfg.width, cfg.heads, cfg.intermediate, cfg.eps) for _ in range(cfg.layers)])


class Bert(nn.Module):
    """BertModel without its pooler; `named_parameters()` gives BertModel's names and order."""

    def __init__(self, variant="bert_base_uncased"):
        super().__init__()
        self.cfg = cfg = VARIANTS[variant] if isinstance(variant, str) else variant
        self.embeddings = Embeddings(cfg)
        self.encoder = Encoder(cfg)
        # BertPreTrainedModel._init_weights: normal(0, 0.02) matrices and tables, zero biases, unit LayerNorm
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, std=0.02)
            if isinstance(m, nn.Linear):
                nn.init.zeros_(m.bias)

    def hidden(self, ids, attention_mask=None):
        """last_hidden_state [N, L, D] of padded ids [N, L]; attention_mask [N, L] ones / zeros (None: no padding)."""
        n, l = ids.shape
        x = self.embeddings(ids, torch.arange(l).expand(n, l))
        key_mask = None
        if attention_mask is not None:
            key_mask = torch.zeros(n, l, dtype=x.dtype).masked_fill_(attention_mask == 0, float("-inf"))
        for blk in self.encoder.layer:
            x = blk(x, key_mask)
        return x

    def forward(self, ids, attention_mask=None):
        return self.hidden(ids, attention_mask)[:, 0]

    def forward_packed(self, ids_packed, lens):
        """ids_packed [sum(lens)]: the sequences one after another -> [len(lens), D], the first row of each."""
        lens = [int(v) for v in lens]
        pos = torch.cat([torch.arange(v) for v in lens])
        x = self.embeddings(ids_packed, pos)
        for blk in self.encoder.layer:
            x = blk.forward_packed(x, lens)
        starts = torch.tensor([0] + lens[:-1]).cumsum(0)
        return x[starts]


def randomize_like_trained(module: nn.Module, seed: int):
    """Break the symmetric default init (unit LayerNorm gains, zero biases) and give the attention scores a spread of
    about one (query / key rows of unit norm in place of the init's 0.02 sqrt(width)): under the init the softmax is
    nearly flat, and a key that should have been masked would hardly show."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if "LayerNorm" in name and leaf == "weight":
                p.add_((0.1 * torch.randn(p.shape, generator=g)).to(p.dtype))
            elif leaf == "bias":
                p.add_((0.02 * torch.randn(p.shape, generator=g)).to(p.dtype))
            elif ".query." in name or ".key." in name:
                p.mul_(1.0 / (0.02 * p.shape[1] ** 0.5))


def named_shapes(module):
    return [(n, tuple(p.shape)) for n, p in module.named_parameters()]


def state_for_tower(module):
    """name -> tensor of the restatement under BertModel's bare names (what `TextTower.flat_from_state_dict` takes)."""
    return {n: p.detach().clone() for n, p in module.named_parameters()}
