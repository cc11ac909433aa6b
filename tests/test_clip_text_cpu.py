"""The frozen CLIP text tower (`--text_encoder clip`) without a GPU: the restatement's causal block against the
reference's own `ResidualAttentionBlock(..., attn_mask=causal)` (through tests/golden/clip_text_block_small.npz, written
by tools/gen_clip_text_golden.py), causality of the restatement, the library's parameter table (spec-only towers,
bind=False), the cache writer and the argument checks of the Python layer."""
import os

import numpy as np
import pytest
import torch

from clip_text_ref import CausalBlock, TextEncoder as RefEncoder, named_shapes, randomize_like_trained
from conftest import GOLDEN, rel_err


def test_causal_block_matches_the_reference_block(report):
    """tests/clip_text_ref.CausalBlock in float64 on the fixture's input and parameters against what the reference's
    model.py computed in fp32 under its additive -inf mask: within 1e-5 relative (L2), the bound
    tests/test_clip_vit_cpu.py uses for the unmasked block.  Measured with exactly these shapes: 8.6e-8 -- the
    reference's own fp32 rounding."""
    z = np.load(os.path.join(GOLDEN, "clip_text_block_small.npz"))
    names = [str(n) for n in z["names"]]
    blk = CausalBlock(64, int(z["heads"])).double()
    own = dict(blk.named_parameters())
    assert list(own) == names                      # the registration order of the reference's block
    with torch.no_grad():
        for n in names:
            own[n].copy_(torch.from_numpy(z["param." + n]).double())
        x = torch.from_numpy(z["x"]).double()
        assert x.shape == (3, 33, 64)
        y = blk(x)
    e_y = rel_err(y, torch.from_numpy(z["y"]))
    report(f"clip text block vs the reference's ResidualAttentionBlock(64, 2, attn_mask=causal): output {e_y:.1e}")
    assert e_y < 1e-5, e_y
    # the mask matters on this fixture: the unmasked block is far away
    from clip_vit_ref import Block
    plain = Block(64, int(z["heads"])).double()
    plain.load_state_dict(blk.state_dict())
    with torch.no_grad():
        assert rel_err(plain(x), torch.from_numpy(z["y"])) > 1e-2


def test_restatement_is_causal():
    """The hidden state at position t does not change, bit for bit, when ids after t change; the features of a sequence
    therefore depend on nothing behind its end-of-text token."""
    torch.manual_seed(0)
    enc = RefEncoder("clip_text_nano").double()
    randomize_like_trained(enc, 1)
    cfg = enc.model.cfg
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(1, cfg.vocab - 1, (4, cfg.ctx), generator=g)
    cut = [0, 5, 31, cfg.ctx - 1]
    ids2 = ids.clone()
    for r, t in enumerate(cut):
        ids2[r, t + 1:] = torch.randint(1, cfg.vocab - 1, (cfg.ctx - t - 1,), generator=g)
    assert not torch.equal(ids, ids2)
    with torch.no_grad():
        h, h2 = enc.model.hidden(ids), enc.model.hidden(ids2)
    for r, t in enumerate(cut):
        assert torch.equal(h[r, :t + 1], h2[r, :t + 1]), (r, t)
        if t + 1 < cfg.ctx:
            assert not torch.equal(h[r, t + 1:], h2[r, t + 1:])
    # end-of-text (the largest id) at `cut`: the features ignore what follows it
    for r, t in enumerate(cut):
        ids[r, t] = ids2[r, t] = cfg.vocab - 1
    with torch.no_grad():
        assert torch.equal(enc(ids), enc(ids2))


CLIP_NAMES_L0 = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight",
                 "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight",
                 "ln_2.bias"]


@pytest.mark.parametrize("variant,numel,feat,ctx,vocab", [("clip_text_b32", 63_428_096, 512, 77, 49408),
                                                          ("clip_text_micro", None, 24, 77, 512),
                                                          ("clip_text_nano", None, 8, 33, 64)])
def test_spec_only_tower_reports_the_clip_table(variant, numel, feat, ctx, vocab):
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower(variant, max_batch=4, compute_dtype="bf16", bind=False)
    tab = tw.param_table()
    ref = named_shapes(RefEncoder(variant)) if variant != "clip_text_b32" else None
    assert tw.feature_dim == feat and tw.context == ctx and tw.vocab == vocab
    names = [n for n, _, _ in tab]
    shapes = {n: tuple(s) for n, s, _ in tab}
    width = shapes["model.positional_embedding"][1]
    layers = 1 + max(int(n.split(".")[3]) for n in names if n.startswith("model.transformer.resblocks."))
    want = ["model.positional_embedding", "model.text_projection"]
    for l in range(layers):
        want += ["model.transformer.resblocks.%d.%s" % (l, s) for s in CLIP_NAMES_L0]
    want += ["model.token_embedding.weight", "model.ln_final.weight", "model.ln_final.bias"]
    assert names == want
    assert shapes["model.positional_embedding"] == (ctx, width) and shapes["model.text_projection"] == (width, feat)
    assert shapes["model.token_embedding.weight"] == (vocab, width)
    assert shapes["model.transformer.resblocks.0.attn.in_proj_weight"] == (3 * width, width)
    assert shapes["model.transformer.resblocks.0.mlp.c_fc.weight"] == (4 * width, width)
    sizes = [int(np.prod(s)) for _, s, _ in tab]
    assert [o for _, _, o in tab] == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    assert tw.param_numel == sum(sizes)
    if numel is not None:
        # 151,277,313 (whole CLIP ViT-B/32) - 87,849,216 (the visual tower) - 1 (logit_scale)
        assert tw.param_numel == numel == 151_277_313 - 87_849_216 - 1 and layers == 12 and width == 512
    if ref is not None:
        assert [(n, tuple(s)) for n, s, _ in tab] == ref          # the restatement registers CLIP's order
    assert tw.workspace_bytes > 0
    tw.close()


def test_unknown_variant_and_dtype_fail_loudly():
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    with pytest.raises(RuntimeError, match="invalid argument"):
        TextTower("no_such_tower", bind=False)
    with pytest.raises(RuntimeError, match="invalid argument"):
        TextTower("clip_text_nano", max_batch=0, bind=False)
    with pytest.raises(ValueError, match="compute_dtype"):
        TextTower("clip_text_nano", compute_dtype="bf16x2", bind=False)


def test_write_embed_cache_round_trips_exactly(tmp_path):
    from types import SimpleNamespace
    from multimodal_dataset_distillation_amd.embed_cache import (EMBED_KEY, embed_cache_filename, load_embed_cache,
                                                                 write_embed_cache)
    g = torch.Generator().manual_seed(3)
    arr = torch.randn(7, 24, generator=g)
    args = SimpleNamespace(dataset="flickr", text_encoder="clip", embed_dir=str(tmp_path))
    for file_type, who in (("text", args), ("train_text", ("flickr", "clip"))):
        path = write_embed_cache(who, file_type, arr if file_type == "text" else arr.double().numpy(), str(tmp_path))
        assert path == os.path.join(str(tmp_path), embed_cache_filename("flickr", "clip", file_type))
        with np.load(path, allow_pickle=False) as z:
            assert z.files == [EMBED_KEY] and z[EMBED_KEY].dtype == np.float32
        back = load_embed_cache(args, file_type)
        assert back.dtype == torch.float32 and torch.equal(back, arr)
    with pytest.raises(ValueError):
        write_embed_cache(args, "test", arr, str(tmp_path))
    with pytest.raises(ValueError):
        write_embed_cache(args, "text", arr[0], str(tmp_path))


def test_ids_are_checked_before_anything_runs():
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower("clip_text_nano", max_batch=4, compute_dtype="f32", bind=False)
    ok = torch.zeros(2, tw.context, dtype=torch.int64)
    assert tw.check_ids(ok).dtype == torch.int32
    with pytest.raises(ValueError, match="integers"):
        tw.encode(ok.float())
    with pytest.raises(ValueError, match=r"\[n, 33\]"):
        tw.encode(torch.zeros(2, tw.context + 1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[n, 33\]"):
        tw.encode(torch.zeros(tw.context, dtype=torch.int64))
    for bad in (-1, tw.vocab, tw.vocab + 5):
        ids = ok.clone()
        ids[1, 3] = bad
        with pytest.raises(ValueError, match=r"\[0, 64\)"):
            tw.encode(ids)
    ids = ok.clone()
    ids[0, 0], ids[1, -1] = 0, tw.vocab - 1               # the first and the last entry are fine
    tw.check_ids(ids.numpy())
    tw.close()


def test_state_dict_is_matched_by_name(tmp_path):
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower("clip_text_nano", max_batch=4, compute_dtype="f32", bind=False)
    torch.manual_seed(4)
    enc = RefEncoder("clip_text_nano")
    randomize_like_trained(enc, 5)
    sd = {k: v.detach().clone() for k, v in enc.model.state_dict().items()}        # the `clip` package's keys: no prefix
    want = torch.cat([p.detach().reshape(-1) for _, p in enc.named_parameters()])
    assert torch.equal(tw.flat_from_state_dict(sd), want)
    # any order, fp16, the `model.` prefix, the other half of CLIP beside it
    mixed = {"logit_scale": torch.tensor(4.6), "visual.proj": torch.zeros(3, 2), "visual.conv1.weight": torch.zeros(2, 3, 4, 4)}
    for k in reversed(list(sd)):
        mixed["model." + k] = sd[k].half()
    got = tw.flat_from_state_dict(mixed)
    assert got.dtype == torch.float32 and torch.equal(got, want.half().float())
    lacking = dict(sd); del lacking["ln_final.bias"]
    with pytest.raises(ValueError, match="lacks 'ln_final.bias'"):
        tw.flat_from_state_dict(lacking)
    wrong = dict(sd); wrong["text_projection"] = sd["text_projection"].t().contiguous()
    with pytest.raises(ValueError, match="text_projection.*shape"):
        tw.flat_from_state_dict(wrong)
    # the same two through a file, before any GPU is asked for
    path = str(tmp_path / "state.pt")
    torch.save(lacking, path)
    with pytest.raises(ValueError, match="lacks"):
        tw.load_state_dict_file(path)
    torch.save(wrong, path)
    with pytest.raises(ValueError, match="shape"):
        tw.load_state_dict_file(path)
    with pytest.raises(ValueError, match="float32"):
        tw.load_flat(want[:-1])
    tw.close()
