"""The frozen CLIP text tower on the GPU (csrc/attn_causal.hip, csrc/text_tower.hip; `mdd_op_attention_causal`,
`mdd_op_token_embed`, `mdd_op_eot_gather`, `mdd_text_tower_*`, text_tower.py, embed_text.py) against float64: the three
new kernels at the op level, the tower against the restatement tests/clip_text_ref.py (whose block
tests/test_clip_text_cpu.py pins to the reference's own code), causality bit for bit, and the cache writer end to end."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from clip_text_ref import TextEncoder as RefEncoder, randomize_like_trained
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": 0, "bf16": 1}
ST = {"f32": torch.float32, "bf16": torch.bfloat16}


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _lib():
    from multimodal_dataset_distillation_amd import _lib as mod
    return mod, mod.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------- causal attention
def ref_causal_attention(qkv, heads):
    """float64: out[i] = softmax(scale * q_i . K[0..i]) V[0..i] on the fused [n, t, 3, heads, 64] tensor."""
    n, t, _ = qkv.shape
    d = qkv.shape[2] // 3
    hd = d // heads
    q, k, v = qkv.double().reshape(n, t, 3, heads, hd).permute(2, 0, 3, 1, 4)
    mask = torch.full((t, t), float("-inf"), dtype=torch.float64).triu_(1)
    p = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5 + mask, dim=-1)
    return (p @ v).transpose(1, 2).reshape(n, t, d)


def run_causal(dtype, qkv_dev, n, tokens, heads):
    mod, lib = _lib()
    out = torch.full((n, tokens, heads * 64), float("nan"), device=DEV, dtype=ST[dtype])     # must be fully overwritten
    mod.check(lib.mdd_op_attention_causal(DT[dtype], n, tokens, heads, 64 ** -0.5, P(qkv_dev), P(out), _stream()))
    torch.cuda.synchronize()
    return out


# caps: f32 the OP_TOL["f32"] of tests/test_gpu_clip_vit.py (2e-6), bf16 the 2.5e-2 of tests/test_gpu_attention.py for its
# mode 0 (the probabilities enter the second product rounded to bf16); the asserted guard is min(cap, 2 x the largest
# value measured on MI355X over the twelve shapes).  Measured: f32 <= 2.2e-7 (128 tokens), bf16 <= 1.8e-3
ATTN_F32_MEASURED, ATTN_BF16_MEASURED = 2.2e-7, 1.8e-3
ATTN_TOL = {"f32": min(2e-6, 2 * ATTN_F32_MEASURED), "bf16": min(2.5e-2, 2 * ATTN_BF16_MEASURED)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("tokens", [1, 31, 32, 33, 77, 128])
def test_causal_attention_matches_float64(dtype, heads, tokens, report):
    n = 3
    g = torch.Generator().manual_seed(100 * tokens + heads)
    qkv = (torch.randn(n, tokens, 3 * heads * 64, generator=g) * 1.5).bfloat16()       # bf16-exact in either storage type
    o_ref = ref_causal_attention(qkv, heads)
    out = run_causal(dtype, qkv.to(DEV, ST[dtype]).contiguous(), n, tokens, heads)
    assert torch.isfinite(out.float()).all()
    e = rel_err(out.float(), o_ref)
    # row 0 attends to itself alone: it is V[0], whatever the scores are
    v0 = qkv.reshape(n, tokens, 3, heads * 64)[:, 0, 2].float()
    assert torch.equal(out[:, 0].float().cpu(), v0)
    report(f"causal attention {dtype} n={n} tokens={tokens} heads={heads}: O {e:.2e}")
    assert e < ATTN_TOL[dtype], e


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tokens,cut", [(77, 40), (33, 31), (128, 5)])
def test_masked_keys_reach_neither_the_maximum_nor_the_sum(dtype, tokens, cut):
    """The KEY rows after `cut` times 1e3 (the values left alone: 0 * a huge V must stay finite as well): output rows
    0 .. cut are bit-identical to the unscaled run.  A maximum or a denominator that saw a masked key would move them (the
    scaled scores are ~1e3 times larger than any unmasked one)."""
    n, heads = 3, 3
    g = torch.Generator().manual_seed(tokens)
    qkv = (torch.randn(n, tokens, 3, heads * 64, generator=g) * 1.5).bfloat16()
    big = qkv.clone()
    big[:, cut + 1:, 1] = (big[:, cut + 1:, 1].float() * 1e3).bfloat16()
    assert not torch.equal(big, qkv)
    a = run_causal(dtype, qkv.reshape(n, tokens, -1).to(DEV, ST[dtype]).contiguous(), n, tokens, heads)
    b = run_causal(dtype, big.reshape(n, tokens, -1).to(DEV, ST[dtype]).contiguous(), n, tokens, heads)
    assert torch.isfinite(b.float()).all()
    assert torch.equal(a[:, :cut + 1], b[:, :cut + 1])
    assert not torch.equal(a[:, cut + 1:], b[:, cut + 1:])


def test_causal_attention_refuses_what_it_cannot_take():
    mod, lib = _lib()
    x = torch.zeros(1, 129, 3 * 64, device=DEV)
    for tokens in (0, 129):
        assert lib.mdd_op_attention_causal(0, 1, tokens, 1, 0.125, P(x), P(x), _stream()) != 0
        assert b"invalid argument" in lib.mdd_last_error()
    assert lib.mdd_op_attention_causal(2, 1, 8, 1, 0.125, P(x), P(x), _stream()) != 0       # bf16x2 is no storage type
    assert lib.mdd_op_attention_causal(0, 1, 8, 1, 0.125, None, P(x), _stream()) != 0


# ---------------------------------------------------------------------------------------------- token embedding
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_token_embed_is_exact(dtype):
    """E = table[ids] + pos: the fp32 sum itself in f32 storage, that sum rounded once (to nearest even) in bf16."""
    mod, lib = _lib()
    n, ctx, width, vocab = 3, 33, 72, 50          # 33 x 72: rows that end inside a 256-thread block
    g = torch.Generator().manual_seed(7)
    table, pos = torch.randn(vocab, width, generator=g), torch.randn(ctx, width, generator=g)
    ids = torch.randint(0, vocab, (n, ctx), generator=g, dtype=torch.int32)
    ids[0, 0], ids[0, 1], ids[2, -1] = 0, vocab - 1, vocab - 1        # the first and the last entry of the vocabulary
    td, pd = table.to(DEV), pos.to(DEV)
    want = (table[ids.long()] + pos).to(ST[dtype])
    out = torch.full((n, ctx, width), float("nan"), device=DEV, dtype=ST[dtype])
    mod.check(lib.mdd_op_token_embed(DT[dtype], n, ctx, width, vocab, P(ids.to(DEV)), P(td), P(pd), P(out), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    # ids outside the table are clamped into it: vocab + 5 reads the last row, -1 the first; nothing else is touched
    bad = ids.clone()
    bad[1, 4], bad[1, 5] = vocab + 5, -1
    clamped = bad.clone()
    clamped[1, 4], clamped[1, 5] = vocab - 1, 0
    pad = 256
    buf = torch.full((pad + n * ctx * width + pad,), float("nan"), device=DEV, dtype=ST[dtype])
    mod.check(lib.mdd_op_token_embed(DT[dtype], n, ctx, width, vocab, P(bad.to(DEV)), P(td), P(pd), P(buf[pad:]), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(buf[pad:pad + n * ctx * width].cpu().reshape(n, ctx, width), (table[clamped.long()] + pos).to(ST[dtype]))
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n * ctx * width:]).all()
    assert torch.equal(td.cpu(), table) and torch.equal(pd.cpu(), pos)
    assert lib.mdd_op_token_embed(DT[dtype], n, ctx, width + 1, vocab, P(ids.to(DEV)), P(td), P(pd), P(out), _stream()) != 0


# ---------------------------------------------------------------------------------------------- EOT gather
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("ctx", [33, 77])         # less than one wave of positions; more than one
def test_eot_gather_is_exact(dtype, ctx):
    """The row at the FIRST position of the largest id (torch.argmax), copied to fp32; with a second tensor, their fp32 sum."""
    mod, lib = _lib()
    width = 72
    g = torch.Generator().manual_seed(ctx)
    rows = []
    r = torch.randint(1, 90, (ctx,), generator=g); r[0] = 99; rows.append(r)                   # the maximum at position 0
    r = torch.randint(1, 90, (ctx,), generator=g); r[-1] = 99; rows.append(r)                  # at the last position
    r = torch.randint(1, 90, (ctx,), generator=g); r[9] = r[20] = r[ctx - 2] = 99; rows.append(r)   # duplicated: the first wins
    rows.append(torch.zeros(ctx, dtype=torch.int64))                                           # all zero: position 0
    r = torch.randint(1, 90, (ctx,), generator=g); r[ctx - 3] = 99; r[ctx - 2:] = 0; rows.append(r)   # padded as clip.tokenize pads
    ids = torch.stack(rows).to(torch.int32)
    n = ids.shape[0]
    at = ids.long().argmax(dim=-1)
    assert at.tolist() == [0, ctx - 1, 9, 0, ctx - 3]
    x = torch.randn(n, ctx, width, generator=g).to(ST[dtype])
    b = torch.randn(n, ctx, width, generator=g).to(ST[dtype])
    xd, bd, idd = x.to(DEV), b.to(DEV), ids.to(DEV)
    for second in (None, bd):
        out = torch.full((n, width), float("nan"), device=DEV)
        mod.check(lib.mdd_op_eot_gather(DT[dtype], n, ctx, width, P(idd), P(xd), P(second), P(out), _stream()))
        torch.cuda.synchronize()
        want = x[torch.arange(n), at].float()
        if second is not None:
            want = want + b[torch.arange(n), at].float()
        assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------- the tower
@functools.lru_cache(maxsize=None)
def oracle(variant):
    """The float64 restatement with trained-like parameters, its flat fp32 parameter vector, ids whose end-of-text token
    (the largest id) lands at varied positions with clip.tokenize's zero padding behind it, and its features."""
    torch.manual_seed(11)
    enc = RefEncoder(variant)
    randomize_like_trained(enc, 12)
    cfg = enc.model.cfg
    n = 3 if variant == "clip_text_b32" else 5
    g = torch.Generator().manual_seed(13)
    ids = torch.randint(1, cfg.vocab - 2, (n, cfg.ctx), generator=g)
    ids[:, 0] = cfg.vocab - 2                                          # start-of-text
    eot = [0, cfg.ctx - 1, 7, cfg.ctx // 2, 32][:n]
    for r, t in enumerate(eot):
        ids[r, t] = cfg.vocab - 1
        ids[r, t + 1:] = 0
    flat = torch.cat([p.detach().reshape(-1) for _, p in enc.named_parameters()]).float()
    with torch.no_grad():
        want = enc.double()(ids)
    enc.float()
    return enc, flat, ids, tuple(eot), want


# caps: the project's forward-pass figures (PASS_TOL of tests/test_gpu_clip_vit.py: 1e-5 f32, 3e-2 bf16, relative L2); the
# asserted guard is min(cap, 2 x the largest value measured on MI355X over micro, nano and b32).
# Measured: f32 micro 6.2e-7, nano 5.3e-7, b32 1.4e-6; bf16 micro 6.7e-3, nano 7.1e-3, b32 1.03e-2
TOWER_F32_MEASURED, TOWER_BF16_MEASURED = 1.4e-6, 1.03e-2
TOWER_TOL = {"f32": min(1e-5, 2 * TOWER_F32_MEASURED), "bf16": min(3e-2, 2 * TOWER_BF16_MEASURED)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["clip_text_micro", "clip_text_nano", "clip_text_b32"])
def test_tower_matches_the_restatement(variant, dtype, report):
    """micro / nano: 5 sequences through max_batch = 2 (two full calls and a ragged one); b32: its real geometry, 3
    sequences in one call."""
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    enc, flat, ids, eot, want = oracle(variant)
    tw = TextTower(variant, max_batch=3 if variant == "clip_text_b32" else 2, compute_dtype=dtype)
    assert tw.param_numel == flat.numel() and tw.feature_dim == want.shape[1]
    tw.load_flat(flat)
    y = tw.encode(ids)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(want.shape) and torch.isfinite(y).all()
    e = rel_err(y, want)
    per = [rel_err(y[r], want[r]) for r in range(len(eot))]
    report(f"{variant} text tower {dtype}: features {e:.2e} | per sequence (EOT at {list(eot)}) " + " ".join(f"{v:.1e}" for v in per))
    assert e < TOWER_TOL[dtype], (e, per)
    tw.close()


@pytest.mark.parametrize("variant", ["clip_text_micro", "clip_text_nano"])
def test_tower_features_ignore_what_follows_the_end_of_text(variant):
    """f32: the features of a sequence do not change by a bit when the ids behind its end-of-text token change."""
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    enc, flat, ids, eot, _ = oracle(variant)
    cfg = enc.model.cfg
    g = torch.Generator().manual_seed(14)
    other = ids.clone()
    for r, t in enumerate(eot):
        other[r, t + 1:] = torch.randint(0, cfg.vocab - 1, (cfg.ctx - t - 1,), generator=g)     # never the largest id again
    assert not torch.equal(other, ids)
    tw = TextTower(variant, max_batch=2, compute_dtype="f32")
    tw.load_flat(flat)
    a, b = tw.encode(ids), tw.encode(other)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    tw.close()


def test_embed_text_writes_the_cache_the_loader_reads(tmp_path, report):
    """embed_text (the reference's textprocess_train for clip) with the micro variant: token file + saved state dict ->
    {dataset}_clip_train_text_embed.npz == TextTower.encode, read back by load_embed_cache."""
    from types import SimpleNamespace
    from multimodal_dataset_distillation_amd import embed_text
    from multimodal_dataset_distillation_amd.embed_cache import load_embed_cache
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    enc, flat, ids, eot, want = oracle("clip_text_micro")
    tok, wts = str(tmp_path / "ids.npy"), str(tmp_path / "state.pt")
    np.save(tok, ids.numpy())
    sd = {k: v.detach().half() if v.dim() == 2 else v.detach().clone() for k, v in enc.model.state_dict().items()}
    sd["logit_scale"] = torch.tensor(4.6052)
    sd["visual.class_embedding"] = torch.zeros(8)
    torch.save(sd, wts)
    args = embed_text.build_parser().parse_args(
        ["--dataset", "flickr", "--file_type", "train_text", "--tokens", tok, "--clip_weights", wts, "--embed_dir",
         str(tmp_path), "--chunk", "2", "--compute_dtype", "f32", "--variant", "clip_text_micro"])
    path = embed_text.main(args)
    assert os.path.basename(path) == "flickr_clip_train_text_embed.npz"
    back = load_embed_cache(SimpleNamespace(dataset="flickr", text_encoder="clip"), "train_text", str(tmp_path))
    tw = TextTower("clip_text_micro", max_batch=2, compute_dtype="f32")
    tw.load_state_dict_file(wts)
    y = tw.encode(ids).cpu()
    tw.close()
    assert back.dtype == torch.float32 and torch.equal(back, y)
    # the file holds its matrices in fp16: the cache is the restatement's features at those rounded weights
    import copy
    enc16 = copy.deepcopy(enc)
    with torch.no_grad():
        for p in enc16.parameters():
            if p.dim() == 2:
                p.copy_(p.half().float())
        want16 = enc16.double()(ids)
    e = rel_err(back, want16)
    report(f"embed_text clip_text_micro f32 from a state dict with fp16 matrices vs the restatement at those weights: {e:.2e}")
    assert e < TOWER_TOL["f32"] and rel_err(want16, want) > 10 * TOWER_TOL["f32"], e
