"""The engine and the op-level entry points pack the same bits.

Eng::build and mdd_op_weight_std fill their WsDesc tables with one builder (ws_desc_fill, csrc/ws.hip), the ViT branch of
Eng::build and mdd_op_lin_pack their LinPackDesc tables with another (lin_pack_desc, csrc/vit.hip), and each pair launches
one kernel.  So the packed weights an engine holds after a forward pass (buffers wf / wt, and wf_t / wt_t after a tangent
forward) must be bit-equal to what the op writes for the same layers -- otherwise tests/test_gpu_head_ws.py and
tests/test_gpu_edge_ops.py would be testing descriptors the engine does not use.  What differs between the two callers is
the parameter layout alone: the engine's theta holds {weight, bias, gain} per conv and whatever else the network has, the
ops' theta {weight, gain} per conv, or {weight, bias} per linear, back to back.

nf_regnet_tiny has the group counts 5, 11, 23 and 27 and a first conv padded from 3 to 8 input channels: the places where
the running row / tile counters of the descriptors can go wrong."""
import ctypes as C
import math

import pytest
import torch

from test_gpu_small_ops import P, _lib, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f32": 0, "bf16": 1}
BATCH, SIZE, D_TXT = 2, 32, 16
# NfCfg of both convolutional variants (csrc/engine.hip get_cfg): timm's _nonlin_gamma['silu'] and std_conv_eps
GAMMA, EPS = 1.7881293296813965, 1e-5


def _engine(variant, dtype):
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    return UnrollEngine(variant, batch=BATCH, num_queries=BATCH, image_size=SIZE, d_txt=D_TXT, syn_steps=1, dtype=dtype)


def _thetas(eng, seed):
    """theta and a tangent direction: every gain is drawn around 1 (a gain of exactly 1 would hide a wrong off_g)"""
    g = torch.Generator().manual_seed(seed)
    th, th_t = 0.1 * torch.randn(eng.P_img, generator=g), 0.1 * torch.randn(eng.P_img, generator=g)
    for name, shape, off in eng.param_table("img"):
        if name.endswith(".gain"):
            th[off:off + shape[0]] = 1.0 + 0.3 * torch.randn(shape[0], generator=g)
    return th.to(DEV), th_t.to(DEV)


def _engine_packed(eng, th, th_t):
    """the four packed buffers after one forward and one tangent forward"""
    g = torch.Generator().manual_seed(5)
    image = torch.randn(BATCH, 3, SIZE, SIZE, generator=g).to(DEV)
    eng.img_forward(0, th, image)
    torch.cuda.synchronize()
    wf, wt = eng.buffer("wf", -2).clone(), eng.buffer("wt", -2).clone()
    eng.img_tangent_forward(0, th, th_t)
    torch.cuda.synchronize()
    return wf, wt, eng.buffer("wf_t", -2).clone(), eng.buffer("wt_t", -2).clone()


def _assert_same(eng_bufs, op, numel):
    """op(tangent, wf, wt, wf_t, wt_t) fills zeroed buffers; they must be the engine's, bit for bit"""
    wf, wt, wf_t, wt_t = eng_bufs
    assert wf.numel() == numel, ("the op's layers do not cover the engine's packed buffer", wf.numel(), numel)
    new = lambda: torch.zeros_like(wf)
    a, b = new(), new()
    op(False, a, b, None, None)
    torch.cuda.synchronize()
    assert torch.equal(a, wf), "wf"
    assert torch.equal(b, wt), "wt"
    a, b, c, d = new(), new(), new(), new()
    op(True, a, b, c, d)
    torch.cuda.synchronize()
    assert torch.equal(a, wf) and torch.equal(b, wt), "wf / wt of the tangent call"
    assert torch.equal(c, wf_t), "wf_t"
    assert torch.equal(d, wt_t), "wt_t"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["nfnet_tiny", "nf_regnet_tiny"])
def test_weight_std_packs_what_the_engine_packs(variant, dtype):
    from multimodal_dataset_distillation_amd._lib import MddWsConv, check
    eng = _engine(variant, dtype)
    table = eng.param_table("img")
    th, th_t = _thetas(eng, 11)
    by_name = {name: (shape, off) for name, shape, off in table}
    convs, pieces, pieces_t, numel = [], [], [], 0
    for name, shape, off in table:                      # table order is the engine's conv order
        if not name.endswith(".weight") or name[:-7] + ".gain" not in by_name:
            continue
        cout, cin_g, k, _ = shape
        # a block's grouped 3x3 convs (conv2, conv2b) map the mid channels onto themselves; every other conv has one group
        cin = cout if ".stages." in name and ".conv2" in name else cin_g
        assert cin % cin_g == 0
        cin_pad = max(cin, 8)
        convs.append((cout, cin, k, cin // cin_g, cin_pad))
        off_g = by_name[name[:-7] + ".gain"][1]
        for src, dst in ((th, pieces), (th_t, pieces_t)):
            dst += [src[off:off + math.prod(shape)], src[off_g:off_g + cout]]
        numel += cout * k * k * (cin_pad // (cin // cin_g))
    assert len(convs) > 10 and any(c[3] > 1 for c in convs) and convs[0][1] == 3
    if variant == "nf_regnet_tiny":
        assert {5, 11, 23, 27} <= {c[3] for c in convs}
    o_th, o_th_t = torch.cat(pieces).contiguous(), torch.cat(pieces_t).contiguous()
    cv = (MddWsConv * len(convs))(*[MddWsConv(*c) for c in convs])

    def op(tangent, wf, wt, wf_t, wt_t):
        check(_lib().mdd_op_weight_std(DT[dtype], 0, len(convs), cv, GAMMA, EPS, P(o_th), P(o_th_t) if tangent else None,
                                       P(wf), P(wt), P(wf_t), P(wt_t), None, None, None, _stream()))

    _assert_same(_engine_packed(eng, th, th_t), op, numel)
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["vit_micro", "clip_vit_micro"])
def test_lin_pack_packs_what_the_engine_packs(variant, dtype):
    from multimodal_dataset_distillation_amd._lib import check
    eng = _engine(variant, dtype)
    table = eng.param_table("img")
    th, th_t = _thetas(eng, 13)
    shapes, pieces, pieces_t, numel = [], [], [], 0
    for i, (name, shape, off) in enumerate(table):      # table order is the engine's order of linears
        # the linears: the patch convolution [out, 3, p, p] and every [out, in] matrix called a weight (not CLIP's `proj`
        # and `positional_embedding`, which the engine does not pack)
        if not name.endswith("weight") or len(shape) not in (2, 4):
            continue
        out, inn = shape[0], math.prod(shape[1:])
        shapes += [out, inn]
        nxt = table[i + 1] if i + 1 < len(table) else ("", (), 0)
        has_bias = nxt[0].endswith("bias") and tuple(nxt[1]) == (out,)
        assert has_bias or "conv1" in name, name        # CLIP's patch convolution has no bias: the op's slot gets a dummy
        for src, dst in ((th, pieces), (th_t, pieces_t)):
            dst += [src[off:off + out * inn], src[nxt[2]:nxt[2] + out] if has_bias else torch.zeros(out, device=DEV)]
        numel += out * inn
    assert len(shapes) // 2 == 1 + 4 * 2                # patch embedding + four linears in each of the two blocks
    o_th, o_th_t = torch.cat(pieces).contiguous(), torch.cat(pieces_t).contiguous()
    sh = (C.c_int32 * len(shapes))(*shapes)

    def op(tangent, wf, wt, wf_t, wt_t):
        check(_lib().mdd_op_lin_pack(DT[dtype], len(shapes) // 2, sh, P(o_th), P(o_th_t) if tangent else None, P(wf), P(wt),
                                     P(wf_t), P(wt_t), _stream()))

    _assert_same(_engine_packed(eng, th, th_t), op, numel)
    eng.close()
