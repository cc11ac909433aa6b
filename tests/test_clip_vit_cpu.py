"""The CLIP ViT-B/32 image tower (`--image_encoder clip`) without a GPU: the restatement's block against the reference's
own `ResidualAttentionBlock` (through tests/golden/clip_block_small.npz, written by tools/gen_clip_golden.py), the
engine's parameter table against the restatement (spec-only engines, bind=False), the expert-file loader's slicing of a
whole-model snapshot, and the initialisation of the new table."""
import os

import numpy as np
import pytest
import torch

from clip_vit_ref import Block, ImageEncoder as RefEncoder
from conftest import GOLDEN, rel_err


def test_block_matches_the_reference_block(report):
    """tests/clip_vit_ref.Block in float64 on the fixture's input and parameters against what the reference's model.py
    computed in fp32: output and every gradient within 1e-5 relative (L2).  Measured with exactly these shapes: output
    8.5e-8, worst gradient tensor 4.3e-7 -- what remains is the reference's own fp32 rounding."""
    z = np.load(os.path.join(GOLDEN, "clip_block_small.npz"))
    names = [str(n) for n in z["names"]]
    blk = Block(64, int(z["heads"])).double()
    own = dict(blk.named_parameters())
    assert list(own) == names                      # the registration order of the reference's block
    with torch.no_grad():
        for n in names:
            own[n].copy_(torch.from_numpy(z["param." + n]).double())
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    y = blk(x)
    grads = torch.autograd.grad(y, [x] + [own[n] for n in names], torch.from_numpy(z["w"]).double())
    e_y = rel_err(y, torch.from_numpy(z["y"]))
    e_g = {n: rel_err(g, torch.from_numpy(z["grad." + n])) for n, g in zip(["x"] + names, grads)}
    worst = max(e_g, key=e_g.get)
    report(f"clip block vs the reference's ResidualAttentionBlock(64, 2): output {e_y:.1e}, worst gradient tensor "
           f"{worst} {e_g[worst]:.1e}")
    assert e_y < 1e-5 and all(v < 1e-5 for v in e_g.values()), (e_y, e_g)


@pytest.mark.parametrize("variant,size,feat,tokens", [("clip_vit_micro", 32, 24, 17), ("clip_vit_b32", 224, 512, 50),
                                                      ("clip_vit_nano", 32, 8, 17)])
def test_parameter_table_is_the_restatements(variant, size, feat, tokens):
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    from multimodal_dataset_distillation_amd.networks import VARIANTS
    from oracle.distill_ref import FlatModule
    assert VARIANTS["clip"] == "clip_vit_b32" and VARIANTS[variant] == variant
    eng = UnrollEngine(variant, batch=4, image_size=size, d_txt=16, syn_steps=1, dtype="bf16", bind=False)
    fm = FlatModule(RefEncoder(variant, img_size=size))
    tab = eng.param_table("img")
    offs = np.concatenate([[0], np.cumsum(fm.numels)[:-1]]).tolist()
    assert [n for n, _, _ in tab] == fm.names
    assert [tuple(s) for _, s, _ in tab] == fm.shapes
    assert [o for _, _, o in tab] == offs
    assert eng.P_img == fm.param_numel and eng.feature_dim == feat
    if variant == "clip_vit_b32":
        assert eng.P_img == 87_849_216
    names = [n for n, _, _ in tab]
    assert all(n.startswith("model.visual.") for n in names)
    assert "model.visual.conv1.weight" in names and "model.visual.conv1.bias" not in names
    assert "model.visual.proj" in names and not any(n.startswith("model.visual.proj.") for n in names)
    shapes = {n: tuple(s) for n, s, _ in tab}
    width = shapes["model.visual.class_embedding"][0]
    assert shapes["model.visual.positional_embedding"] == (tokens, width)
    assert shapes["model.visual.proj"] == (width, feat)
    # the text projection maps to the encoder's features
    assert eng.param_table("txt")[0][1] == (feat, 16)
    eng.close()


def _visual_shapes():
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    eng = UnrollEngine("clip_vit_micro", batch=4, image_size=32, d_txt=16, syn_steps=1, dtype="f32", bind=False)
    shapes = [tuple(s) for _, s, _ in eng.param_table("img")]
    P = eng.P_img
    eng.close()
    return shapes, P


def test_loader_slices_the_visual_run_out_of_a_whole_model_snapshot():
    from multimodal_dataset_distillation_amd.expert_buffer import flatten_trajectories
    shapes, P = _visual_shapes()
    g = torch.Generator().manual_seed(0)

    def snapshot(lead=True, runs=1):
        head = [torch.randn(s, generator=g).half() for s in ((77, 40), (), (40, 24))] if lead else []   # three leading tensors
        vis = [[torch.randn(s, generator=g).half() for s in shapes] for _ in range(runs)]
        tail = [torch.randn(s, generator=g).half() for s in ((48, 40), (120, 40), (120,), (40,))] if lead else []
        return head + [t for v in vis for t in v] + tail, vis[0]
    trajs, want = [], []
    for _ in range(2):
        traj = []
        for _ in range(3):
            snap, vis = snapshot()
            traj.append(snap)
            want.append(torch.cat([t.reshape(-1).float() for t in vis]))
        trajs.append(traj)
    flat = flatten_trajectories(trajs, expect_numel=P, expect_shapes=shapes)
    assert flat.dtype == torch.float32 and flat.shape == (2, 3, P)
    assert torch.equal(flat.reshape(6, P), torch.stack(want))
    # no matching run: a whole-model list of another width
    with pytest.raises(ValueError):
        flatten_trajectories([[[torch.zeros(3, 5) for _ in range(len(shapes) + 4)]]], expect_numel=P, expect_shapes=shapes)
    # the run twice
    with pytest.raises(ValueError):
        flatten_trajectories([[snapshot(runs=2)[0]]], expect_numel=P, expect_shapes=shapes)
    # a plain visual-only list loads as before
    snap, vis = snapshot(lead=False)
    flat = flatten_trajectories([[[t.float() for t in snap]]], expect_numel=P, expect_shapes=shapes)
    assert torch.equal(flat[0, 0], torch.cat([t.reshape(-1).float() for t in vis]))
    with pytest.raises(ValueError):     # ... and still refuses another order
        flatten_trajectories([[[t.float() for t in snap[::-1]]]], expect_numel=P, expect_shapes=shapes)


def test_init_image_params_on_the_clip_table():
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    from multimodal_dataset_distillation_amd.networks import init_image_params
    eng = UnrollEngine("clip_vit_micro", batch=4, image_size=32, d_txt=16, syn_steps=1, dtype="f32", bind=False)
    tab = eng.param_table("img")
    eng.close()
    a = init_image_params(tab, torch.Generator().manual_seed(5))
    b = init_image_params(tab, torch.Generator().manual_seed(5))
    c = init_image_params(tab, torch.Generator().manual_seed(5), trained_like=True)
    assert len(a) == len(tab)
    for (name, shape, _), t, u, v in zip(tab, a, b, c):
        assert tuple(t.shape) == tuple(shape) == tuple(v.shape) and t.dtype == torch.float32, name
        assert torch.isfinite(t).all() and torch.isfinite(v).all(), name
        assert torch.equal(t, u), name                      # a fixed seed reproduces
        if name.endswith("in_proj_bias") or name.endswith("out_proj.bias"):
            assert (t == 0).all() and (v != 0).any(), name  # zero attention biases; trained_like perturbs them
        if ".ln_" in name or "ln_pre" in name or "ln_post" in name:
            assert (t == (1.0 if name.endswith("weight") else 0.0)).all(), name
            assert (v != t).any(), name
    d = dict((n, t) for (n, _, _), t in zip(tab, a))
    w = d["model.visual.transformer.resblocks.0.attn.in_proj_weight"]
    assert float(w.abs().max()) <= (6.0 / (w.shape[0] + w.shape[1])) ** 0.5       # Xavier-uniform bound
    assert 0.5 < float(d["model.visual.proj"].std()) * 64 ** 0.5 < 1.5            # width^-0.5 * randn
