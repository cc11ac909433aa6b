"""NF-RegNet-B1 (`--image_encoder nf_regnet`, reference networks.py:671-672) without a GPU: the engine's parameter
table and workspace plan (spec-only engines, bind=False) against the CPU restatement (tests/nf_regnet_ref.py) and timm's
published size, the Python surface that builds the encoder from that table, and the restatement itself."""
import numpy as np
import pytest
import torch

from nf_regnet_ref import ImageEncoder as RefEncoder, randomize_like_trained


@pytest.mark.parametrize("variant,size", [("nf_regnet_b1", 224), ("nf_regnet_tiny", 64)])
def test_param_table_matches_the_restatement(variant, size):
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    from oracle import distill_ref as dr
    eng = UnrollEngine(variant, batch=4, image_size=size, d_txt=768, syn_steps=1, dtype="bf16", bind=False)
    torch.manual_seed(0)
    enc = RefEncoder(variant)
    fi = dr.FlatModule(enc)
    ft = dr.FlatModule(dr.ProjectionHead(768, enc.model.num_features))
    for tab, fm in ((eng.param_table("img"), fi), (eng.param_table("txt"), ft)):
        assert [t[0] for t in tab] == fm.names
        assert [tuple(t[1]) for t in tab] == [tuple(s) for s in fm.shapes]
        assert [t[2] for t in tab] == np.cumsum([0] + fm.numels[:-1]).tolist()
    assert eng.feature_dim == enc.model.num_features
    eng.close()


def test_nf_regnet_b1_anchors():
    """timm's published nf_regnet_b1: 10.22 M parameters; 66 weight-standardised convolutions, the 1000-way head kept
    (the features are the logits: the projection is 768 -> 1000)."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    eng = UnrollEngine("nf_regnet_b1", batch=4, image_size=224, d_txt=768, syn_steps=1, dtype="bf16", bind=False)
    tab = eng.param_table("img")
    shape = {t[0]: tuple(t[1]) for t in tab}
    assert eng.P_img == 10_223_984
    assert eng.feature_dim == 1000
    assert eng.P_txt == 1_772_000
    assert sum(1 for t in tab if t[0].endswith(".gain")) == 66
    assert tab[0][0] == "model.stem.conv.weight" and tuple(tab[0][1]) == (40, 3, 3, 3)
    assert shape["model.stages.0.0.conv2.weight"] == (40, 8, 3, 3)
    assert shape["model.stages.3.6.conv2.weight"] == (736, 8, 3, 3)
    assert shape["model.final_conv.weight"] == (960, 328, 1, 1)
    assert [t[0] for t in tab[-2:]] == ["model.head.fc.weight", "model.head.fc.bias"]
    assert shape["model.head.fc.weight"] == (1000, 960)
    assert shape["model.stages.3.1.attn.fc1.weight"] == (368, 736, 1, 1)
    assert sum(1 for t in tab if t[0].endswith(".attn.fc1.weight")) == 20
    assert not any(("attn_last" in t[0]) or ("conv2b" in t[0]) for t in tab)
    eng.close()


def test_miniature_covers_the_topology():
    """nf_regnet_tiny: the ratio-1.0 first block, an identity-shortcut block, a stage-0 stride-2 downsample of equal
    width, odd group counts (5, 11, 11, 23, 27), a final conv and a small classifier."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    eng = UnrollEngine("nf_regnet_tiny", batch=4, image_size=64, d_txt=16, syn_steps=1, dtype="f32", bind=False)
    tab = eng.param_table("img")
    shape = {t[0]: tuple(t[1]) for t in tab}
    assert eng.P_img == 311_776 and eng.feature_dim == 24
    groups = [shape[f"model.stages.{s}.{b}.conv2.weight"][0] // 8 for s, b in ((0, 0), (0, 1), (1, 0), (2, 0), (3, 0))]
    assert groups == [5, 11, 11, 23, 27]
    assert shape["model.stages.0.0.downsample.conv.weight"] == (40, 40, 1, 1)
    assert "model.stages.0.1.downsample.conv.weight" not in shape
    assert shape["model.final_conv.weight"] == (240, 120, 1, 1)
    assert shape["model.head.fc.weight"] == (24, 240)
    eng.close()


def test_image_encoder_registers_the_table_in_order():
    from multimodal_dataset_distillation_amd import networks as nw
    assert nw.VARIANTS["nf_regnet"] == "nf_regnet_b1" and nw.VARIANTS["nf_regnet_b1"] == "nf_regnet_b1"
    assert nw.VARIANTS["nf_regnet_tiny"] == "nf_regnet_tiny"
    enc = nw.ImageEncoder(variant="nf_regnet")
    ref = RefEncoder("nf_regnet_b1")
    got = [(n, tuple(p.shape)) for n, p in enc.named_parameters()]
    want = [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
    assert got == want
    assert enc.num_features == 1000
    assert sum(p.numel() for p in enc.parameters()) == 10_223_984
    params = dict(enc.named_parameters())
    # timm init: classifier normal(0, 0.01) with zero bias, conv3 gains zero, other gains one, the squeeze-excite
    # convs kaiming_normal(fan_in, linear) with zero bias
    assert 0.005 < float(params["model.head.fc.weight"].detach().std()) < 0.015
    assert float(params["model.head.fc.bias"].abs().max()) == 0.0
    assert float(params["model.stages.0.0.conv3.gain"].abs().max()) == 0.0
    assert float((params["model.stages.0.0.conv2.gain"] - 1).abs().max()) == 0.0
    w1 = params["model.stages.3.1.attn.fc1.weight"].detach()
    assert abs(float(w1.std()) * 736 ** 0.5 - 1.0) < 0.05
    assert float(params["model.stages.3.1.attn.fc1.bias"].abs().max()) == 0.0


def test_c2_shaped_workspace_fits_hbm():
    """N = 100, syn_steps = 8, bf16 at 224 (BASELINE config 2's shape) below the bound the other encoders are held to."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    eng = UnrollEngine("nf_regnet_b1", batch=100, image_size=224, d_txt=768, syn_steps=8, dtype="bf16", bind=False)
    gib = eng.workspace_bytes / 2**30
    print("nf_regnet_b1 C2-shaped workspace GiB:", gib)
    assert gib < 240
    eng.close()
    e0 = UnrollEngine("nf_regnet_b1", batch=100, image_size=224, d_txt=768, syn_steps=8, dtype="bf16", bind=False,
                      keep_steps=0)
    assert e0.num_slots == 1 and e0.workspace_bytes < eng.workspace_bytes / 3
    e0.close()


def test_the_restatement_itself():
    torch.manual_seed(0)
    enc = RefEncoder("nf_regnet_b1")
    assert sum(p.numel() for p in enc.parameters()) == 10_223_984
    assert sum(1 for n, _ in enc.named_parameters() if n.endswith(".gain")) == 66
    with torch.no_grad():
        assert tuple(enc(torch.randn(2, 3, 224, 224)).shape) == (2, 1000)
    tiny = randomize_like_trained(RefEncoder("nf_regnet_tiny"), 1)
    assert sum(p.numel() for p in tiny.parameters()) == 311_776
    x = torch.randn(3, 3, 64, 64, requires_grad=True)
    y = tiny(x)
    assert tuple(y.shape) == (3, 24)
    ps = list(tiny.parameters())
    g = torch.autograd.grad(y.square().sum(), ps, create_graph=True)
    sum((a * a).sum() for a in g).backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    # the block's parts (what the layer-by-layer GPU check compares) compose to the block
    blk = tiny.model.stages[0][1]
    h = torch.randn(2, 40, 16, 16)
    with torch.no_grad():
        assert torch.allclose(blk.mid_parts(h)[-1], blk(h), atol=1e-6)
