"""NF-RegNet-B1 at its real geometry (224 x 224, 66 convolutions, groups of 8 channels, 1000 logits;
`--image_encoder nf_regnet`): at about 0.6 GMAC per image and pass the CPU restatement (tests/nf_regnet_ref.py) still
finishes a double backward of a small problem, so the full-size network is checked against it directly: the forward
pass and the inner gradient in float64, and one whole outer iteration (reference distill.py:509-606) with the SGD step
against oracle/distill_ref driven with the restatement."""
import ctypes as C

import pytest
import torch

from conftest import rel_err
from nf_regnet_ref import ImageEncoder as RefEncoder, randomize_like_trained

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_oracle(d_txt, seed):
    from oracle import distill_ref as dr
    torch.manual_seed(seed)
    enc = RefEncoder("nf_regnet_b1")
    randomize_like_trained(enc, seed + 1)
    head = dr.ProjectionHead(d_txt, enc.model.num_features)
    with torch.no_grad():
        head.layer_norm.weight.add_(0.1 * torch.randn_like(head.layer_norm.weight))
        head.layer_norm.bias.add_(0.1 * torch.randn_like(head.layer_norm.bias))
    return dr.FlatModule(enc), dr.FlatModule(head)


def test_nf_regnet_b1_forward_and_inner_gradient_against_float64(report):
    """N = 2 in f32 against the restatement evaluated in float64: features and the whole gradient within the project's
    1e-3 bar, the least accurate parameter tensor reported.  Measured on MI355X: features 7.2e-7, gradient 7.6e-7, worst
    tensor model.stages.1.1.attn.fc2.weight 1.4e-6."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    from torch.func import vjp
    n, size = 2, 224
    fi, _ = make_oracle(768, 9)
    th = fi.flat_param()
    assert th.numel() == 10_223_984
    g = torch.Generator().manual_seed(10)
    x = torch.randn(n, 3, size, size, generator=g)
    w = torch.randn(n, 1000, generator=g)
    eng = UnrollEngine("nf_regnet_b1", batch=n, num_queries=n, image_size=size, d_txt=768, syn_steps=1, dtype="f32")
    y = eng.img_forward(0, th.to(DEV), x.to(DEV)).cpu()
    gth = eng.img_backward(0, th.to(DEV), w.to(DEV)).cpu()
    torch.cuda.synchronize()
    tab = eng.param_table("img")
    eng.close()
    fi.module.double()
    y64, pull = vjp(lambda t: fi(x.double(), flat_param=t), th.double())
    (g64,) = pull(w.double())
    fi.module.float()
    sl = lambda v, o, s: v[o:o + int(torch.tensor(s).prod())]
    rows = [(nme, rel_err(sl(gth, o, s), sl(g64, o, s))) for nme, s, o in tab]
    worst = max(rows, key=lambda r: r[1])
    e = dict(y=rel_err(y, y64), g_theta=rel_err(gth, g64))
    report("nf_regnet_b1 224 N=2 f32 against float64: " + " ".join(f"{k} {v:.1e}" for k, v in e.items())
           + f" | worst gradient tensor {worst[0]} {worst[1]:.1e}")
    assert e["y"] < 1e-3 and e["g_theta"] < 1e-3, e


def reference_outer_iteration(n=8, K=2, size=224, d_txt=768, seed=31):
    """One outer iteration of the full-size network on the CPU (oracle/distill_ref + the restatement), the expert target
    built as networks.student_move_normalised_targets builds it (a displacement of the size of the student's own K-step
    move, so the grand loss depends on the inner path), and one SGD step that moves the synthetic set by a tenth of its norm."""
    from oracle import distill_ref as dr
    fi, ft = make_oracle(d_txt, seed)
    img, txt = dr.synthetic_inputs(n, size, d_txt, seed=seed + 3)
    g = torch.Generator().manual_seed(seed + 5)
    perms = [torch.randperm(n, generator=g) for _ in range(K)]
    th0i, th0t = fi.flat_param(), ft.flat_param()
    a, b = th0i.clone().requires_grad_(True), th0t.clone().requires_grad_(True)
    l0 = dr.contrastive_loss(fi(img, flat_param=a), ft(txt, flat_param=b), 0.1)
    gi0, gt0 = torch.autograd.grad(l0, [a, b])
    tgi = th0i + float(0.1 * K * gi0.norm() / th0i.numel() ** 0.5) * torch.randn(th0i.shape, generator=g)
    tgt = th0t + float(0.1 * K * gt0.norm() / th0t.numel() ** 0.5) * torch.randn(th0t.shape, generator=g)
    im, tx = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
    lri, lrt = torch.tensor(0.1, requires_grad=True), torch.tensor(0.1, requires_grad=True)
    grand, _ = dr.unrolled_match(fi, ft, im, tx, lri, lrt, th0i, th0t, tgi, tgt, perms)
    gi, gt_, gli, glt = dr.outer_grads(grand, im, tx, lri, lrt)
    step = (float(0.1 * img.norm() / gi.norm()), float(0.1 * txt.norm() / gt_.norm()))
    return dict(img=img, txt=txt, perms=torch.stack(perms), th0i=th0i, th0t=th0t, tgi=tgi, tgt=tgt, step=step,
                grand=grand.detach(), img_after=img - step[0] * gi, txt_after=txt - step[1] * gt_, g_img=gi, g_txt=gt_)


# Measured on MI355X (grand / image_syn_after / text_syn_after / g_img / g_txt):
#   f32     1.2e-7 / 1.9e-7 / 7.7e-7 / 1.9e-6 / 7.7e-6
#   bf16x2  3.8e-6 / 2.4e-6 / 7.7e-6 / 2.4e-5 / 7.7e-5
#   bf16    7.8e-4 / 1.5e-3 / 9.9e-4 / 1.5e-2 / 9.9e-3
# bf16 grand loss: capped by tests/test_gpu_c2.py BF16_C2_FULL["grand"] (6e-3); guard twice the measured value.  The other
# bf16 figures are reported only.
BF16_GRAND = 1.6e-3
assert BF16_GRAND <= 6e-3


def test_nf_regnet_b1_outer_iteration_against_the_oracle(report):
    """N = 8, K = 2 at 224 x 224: grand loss and the synthetic set after the SGD step; f32 and bf16x2 within the 1e-3 bar,
    bf16 finite, its grand loss guarded."""
    from multimodal_dataset_distillation_amd import _lib
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    lib = _lib.load()
    n, K, size, d_txt = 8, 2, 224, 768
    ref = reference_outer_iteration(n, K, size, d_txt)
    assert abs(float(ref["grand"]) - 2.0) > 0.05
    P = lambda t: C.c_void_p(t.data_ptr())
    for dtype in ("f32", "bf16x2", "bf16"):
        eng = UnrollEngine("nf_regnet_b1", batch=n, num_queries=n, image_size=size, d_txt=d_txt, syn_steps=K, dtype=dtype)
        imd, txd = ref["img"].to(DEV).clone(), ref["txt"].to(DEV).clone()
        lr = torch.tensor([0.1, 0.1], device=DEV)
        out = eng.unrolled_match(imd, txd, lr[0:1], lr[1:2], ref["th0i"].to(DEV), ref["th0t"].to(DEV), ref["tgi"].to(DEV),
                                 ref["tgt"].to(DEV), perms=ref["perms"].to(DEV))
        bufs = [torch.zeros_like(imd), torch.zeros_like(txd)]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for p, gr, b, s in ((imd, out["image_syn"], bufs[0], ref["step"][0]), (txd, out["text_syn"], bufs[1], ref["step"][1])):
            _lib.check(lib.mdd_flat_sgd_momentum(P(p), P(gr), P(b), s, 0.5, 1, p.numel(), st))
        torch.cuda.synchronize()
        e = dict(grand=abs(out["grand_loss"].item() - ref["grand"].item()) / abs(ref["grand"].item()),
                 image_syn_after=rel_err(imd, ref["img_after"]), text_syn_after=rel_err(txd, ref["txt_after"]),
                 g_img=rel_err(out["image_syn"], ref["g_img"]), g_txt=rel_err(out["text_syn"], ref["g_txt"]))
        report(f"nf_regnet_b1 outer iteration N={n} K={K} 224 {dtype} (grand {ref['grand'].item():.5f}): "
               + " ".join(f"{k} {float(v):.2e}" for k, v in e.items()))
        assert all(bool(torch.isfinite(t).all()) for t in (imd, txd, out["lr"])), dtype
        if dtype == "bf16":
            assert e["grand"] < BF16_GRAND, e
        else:
            assert e["grand"] < 1e-3 and e["image_syn_after"] < 1e-3 and e["text_syn_after"] < 1e-3, e
        eng.close()
