"""NF-ResNet-50 (`--image_encoder nf_resnet50`, reference networks.py:669-670) without a GPU: the engine's
parameter table and workspace plan (spec-only engines, bind=False) against the CPU restatement (tests/nf_resnet_ref.py)
and timm's published size, and the Python surface that builds the encoder from that table."""
import numpy as np
import pytest
import torch

from nf_resnet_ref import ImageEncoder as RefEncoder


@pytest.mark.parametrize("variant,size", [("nf_resnet50", 224), ("nf_resnet_tiny", 64)])
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
    assert sum(1 for t in eng.param_table("img") if t[0].endswith(".gain")) == \
        sum(1 for m in enc.modules() if isinstance(m, torch.nn.Conv2d))
    eng.close()


def test_nf_resnet50_anchors():
    """timm's published nf_resnet50: 25.56 M parameters, 53 convolutions, the 1000-way head kept (the features are
    the logits: the projection is 768 -> 1000, reference networks.py:818-819)."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    eng = UnrollEngine("nf_resnet50", batch=4, image_size=224, d_txt=768, syn_steps=1, dtype="bf16", bind=False)
    tab = eng.param_table("img")
    assert eng.P_img == 25_557_032
    assert eng.feature_dim == 1000
    assert eng.P_txt == 1_772_000
    assert sum(1 for t in tab if t[0].endswith(".gain")) == 53
    assert tab[0][0] == "model.stem.conv.weight" and tuple(tab[0][1]) == (64, 3, 7, 7)
    assert [t[0] for t in tab[-2:]] == ["model.head.fc.weight", "model.head.fc.bias"]
    assert tuple(tab[-2][1]) == (1000, 2048)
    assert not any(("attn_last" in t[0]) or ("conv2b" in t[0]) or ("final_conv" in t[0]) for t in tab)
    eng.close()


def test_image_encoder_registers_the_table_in_order():
    from multimodal_dataset_distillation_amd import networks as nw
    assert nw.VARIANTS["nf_resnet50"] == "nf_resnet50" and nw.VARIANTS["nf_resnet_tiny"] == "nf_resnet_tiny"
    enc = nw.ImageEncoder(variant="nf_resnet50")
    ref = RefEncoder("nf_resnet50")
    got = [(n, tuple(p.shape)) for n, p in enc.named_parameters()]
    want = [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
    assert got == want
    assert enc.num_features == 1000
    assert sum(p.numel() for p in enc.parameters()) == 25_557_032
    params = dict(enc.named_parameters())
    # timm init: classifier normal(0, 0.01) with zero bias, conv3 gains zero, other gains one
    assert 0.005 < float(params["model.head.fc.weight"].detach().std()) < 0.015
    assert float(params["model.head.fc.bias"].abs().max()) == 0.0
    assert float(params["model.stages.0.0.conv3.gain"].abs().max()) == 0.0
    assert float((params["model.stages.0.0.conv2.gain"] - 1).abs().max()) == 0.0


def test_c2_shaped_workspace_fits_hbm():
    """N = 100, syn_steps = 8, bf16 at 224 (BASELINE config 2's shape) below the NFNet-l0 bound."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    eng = UnrollEngine("nf_resnet50", batch=100, image_size=224, d_txt=768, syn_steps=8, dtype="bf16", bind=False)
    gib = eng.workspace_bytes / 2**30
    print("nf_resnet50 C2-shaped workspace GiB:", gib)
    assert gib < 240
    eng.close()
    # the recompute policy shrinks it the same way as NFNet's
    e0 = UnrollEngine("nf_resnet50", batch=100, image_size=224, d_txt=768, syn_steps=8, dtype="bf16", bind=False,
                      keep_steps=0)
    assert e0.num_slots == 1 and e0.workspace_bytes < eng.workspace_bytes / 3
    e0.close()


def test_image_size_is_checked():
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    UnrollEngine("nf_resnet_tiny", batch=4, image_size=64, d_txt=16, syn_steps=1, dtype="f32", bind=False).close()
    with pytest.raises(RuntimeError, match="image_size must be a multiple of 32"):
        UnrollEngine("nf_resnet_tiny", batch=4, image_size=50, d_txt=16, syn_steps=1, dtype="f32", bind=False)


def test_tangent_set_has_no_input_of_its_own():
    """The tangent passes read the primal slot's input; the tangent set (slot -1) plans none (nor stem columns or
    window index, which are unnamed)."""
    import ctypes as C
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    e = UnrollEngine("nf_resnet_tiny", batch=4, image_size=64, d_txt=16, syn_steps=1, dtype="f32", bind=False)
    off, n, f = C.c_int64(), C.c_int64(), C.c_int()
    assert e.lib.mdd_engine_find_buffer(e.h, b"IN", 0, C.byref(off), C.byref(n), C.byref(f)) == 0
    assert n.value == 4 * 64 * 64 * 8
    assert e.lib.mdd_engine_find_buffer(e.h, b"IN", -1, C.byref(off), C.byref(n), C.byref(f)) != 0
    assert e.lib.mdd_engine_find_buffer(e.h, b"stem.C0", -1, C.byref(off), C.byref(n), C.byref(f)) == 0
    e.close()
