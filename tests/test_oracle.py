"""CPU tests of the oracle (the checker itself): structural anchors of the NFNet restatement, the
restated loop against the committed golden fixtures (which were produced with the reference's own
ReparamModule + ProjectionHead, oracle/gen_golden.py), optimiser semantics, and the restatement against what the reference's own ReparamModule computed
(tests/golden/reparam_reference.npz)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_err
from golden_inputs import reparam_shapes, text_only_theta0, unroll_params
from oracle import distill_ref as dr
from oracle import nfnet_ref as nr


def test_nfnet_l0_structural_anchors():
    m = nr.ImageEncoder("nfnet_l0")
    fm = dr.FlatModule(m)
    assert fm.param_numel == 32_769_488            # + 2304*1000+1000 head = 35,074,488 (timm: 35.07 M)
    assert fm.param_numel + 2304 * 1000 + 1000 == 35_074_488
    assert m.model.num_features == 2304            # reference networks.py:811
    assert len(fm.names) == 57 * 3 + 12 * 4       # 57 ScaledStdConv2d (w,b,gain) + 12 SE (fc1,fc2 w,b)
    assert fm.names[:3] == ["model.stem.conv1.weight", "model.stem.conv1.bias", "model.stem.conv1.gain"]
    assert fm.names[-3:] == ["model.final_conv.weight", "model.final_conv.bias", "model.final_conv.gain"]
    # first block of stage 1: downsample.conv -> conv1 -> conv2 -> conv2b -> conv3 -> attn_last
    blk = [n for n in fm.names if n.startswith("model.stages.1.0.")]
    order = [n.split(".")[4] for n in blk]
    assert order[:3] == ["downsample"] * 3 and order[-4:] == ["attn_last"] * 4
    assert dr.FlatModule(dr.ProjectionHead(768, 2304)).param_numel == 7_087_104
    with torch.no_grad():
        y = m(torch.randn(1, 3, 224, 224))
    assert y.shape == (1, 2304)


def test_weight_standardisation_matches_definition():
    conv = nr.ScaledStdConv2d(8, 16, 3, gamma=nr.GAMMA_SILU, eps=1e-5)
    with torch.no_grad():
        conv.gain.copy_(torch.randn_like(conv.gain))
    w = conv.weight.detach()
    mu = w.mean((1, 2, 3), keepdim=True)
    var = w.var((1, 2, 3), unbiased=False, keepdim=True)
    ref = (w - mu) * torch.rsqrt(var + 1e-5) * conv.gain * (nr.GAMMA_SILU * (8 * 9) ** -0.5)
    assert torch.allclose(conv.standardized_weight(), ref, atol=1e-6)


def test_sgd_momentum_matches_torch():
    p0, g1, g2 = torch.randn(50), torch.randn(50), torch.randn(50)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([q], lr=1000.0, momentum=0.5)
    mine, sgd = p0.clone(), dr.SGDMomentum(1000.0, 0.5)
    for g in (g1, g2):
        q.grad = g.clone()
        opt.step()
        mine = sgd.step(mine, g)
    assert torch.allclose(mine, q.detach(), rtol=1e-6, atol=1e-4)


def test_restated_loop_matches_golden_text_only():
    """golden produced by the reference's ReparamModule(ProjectionHead) + the distill.py loop."""
    g = np.load(os.path.join(GOLDEN, "text_only_unroll.npz"))
    n, d_in, d_out, K = int(g["n"]), int(g["d_in"]), int(g["d_out"]), int(g["K"])
    ft = dr.FlatModule(dr.ProjectionHead(d_in, d_out))
    th0, tgt = text_only_theta0(g), torch.from_numpy(g["target"])
    text = torch.from_numpy(g["text_syn"]).requires_grad_(True)
    s = torch.tensor(float(g["lr_img"]), requires_grad=True)
    lrt = torch.tensor(float(g["lr_txt"]), requires_grad=True)
    tp = [th0.clone().requires_grad_(True)]
    for k in range(K):
        idx = torch.from_numpy(g["perms"][k])
        y = ft(text[idx], flat_param=tp[-1])
        loss = dr.contrastive_loss(torch.from_numpy(g["xs"][k]), y, s)
        assert abs(loss.item() - g["ces"][k]) < 1e-6
        tg = torch.autograd.grad(loss, tp[-1], create_graph=True)[0]
        tp.append(tp[-1] - lrt * tg)
    grand = F.mse_loss(tp[-1], tgt, reduction="sum") / F.mse_loss(th0, tgt, reduction="sum")
    gt, gs, gl = torch.autograd.grad(grand, [text, s, lrt])
    assert abs(grand.item() - float(g["grand"])) < 1e-6
    assert rel_err(gt, torch.from_numpy(g["g_text_syn"])) < 1e-5
    assert abs(gs.item() - float(g["g_lr_img"])) < 1e-5 * abs(float(g["g_lr_img"])) + 1e-9
    assert abs(gl.item() - float(g["g_lr_txt"])) < 1e-5 * abs(float(g["g_lr_txt"])) + 1e-9


def test_restated_loop_matches_golden_tiny_two_iterations():
    g = np.load(os.path.join(GOLDEN, "unroll_tiny.npz"))
    n, size, d_txt, K = int(g["n"]), int(g["size"]), int(g["d_txt"]), int(g["K"])
    enc = nr.ImageEncoder(str(g["variant"]))
    fi = dr.FlatModule(enc)
    ft = dr.FlatModule(dr.ProjectionHead(d_txt, enc.model.num_features))
    T = lambda k: torch.from_numpy(g[k])
    img, txt = T("image_syn0").clone(), T("text_syn0").clone()
    lr = torch.tensor([0.1, 0.1])
    opt = [dr.SGDMomentum(1000.0), dr.SGDMomentum(1000.0), dr.SGDMomentum(1e-3)]
    th0i, th0t, tgi, tgt = unroll_params(g)
    for it in range(2):
        ir, tr = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        li, lt = lr[0].clone().requires_grad_(True), lr[1].clone().requires_grad_(True)
        perms = [torch.from_numpy(p) for p in g["perms"][it]]
        grand, aux = dr.unrolled_match(fi, ft, ir, tr, li, lt, th0i, th0t, tgi, tgt, perms)
        gi, gt, gli, glt = dr.outer_grads(grand, ir, tr, li, lt)
        assert abs(grand.item() - float(g[f"it{it}_grand"])) < 1e-5 * abs(float(g[f"it{it}_grand"]))
        assert rel_err(gi, T(f"it{it}_g_image_syn")) < 1e-4
        assert rel_err(gt, T(f"it{it}_g_text_syn")) < 1e-4
        img, txt = opt[0].step(img, gi), opt[1].step(txt, gt)
        lr = opt[2].step(lr, torch.stack([gli, glt]))
        assert rel_err(img, T(f"it{it}_image_syn_after")) < 1e-4
        assert rel_err(lr, T(f"it{it}_lr_after")) < 1e-5


def test_flat_module_matches_reference_reparam_module():
    """tests/golden/reparam_reference.npz holds the reference's own ReparamModule around the same
    ProjectionHead(16, 24): its parameter table and its output through a given flat theta
    (oracle/gen_golden.py gen_reparam)."""
    g = np.load(os.path.join(GOLDEN, "reparam_reference.npz"))
    torch.manual_seed(0)
    fm = dr.FlatModule(dr.ProjectionHead(16, 24))
    assert tuple(fm.numels) == tuple(g["head_numels"].tolist())
    assert reparam_shapes(g, "head") == fm.shapes
    th, x = torch.from_numpy(g["head_theta"]), torch.from_numpy(g["head_x"])
    assert th.numel() == fm.param_numel
    assert torch.allclose(fm(x, flat_param=th), torch.from_numpy(g["head_y"]), atol=1e-6)


def test_retrieval_oracle_matches_reference_itm_eval_golden():
    """tests/golden/itm_eval_small.npz holds the output of the reference's own itm_eval
    (epoch.py:219-244, executed by oracle/gen_golden.py) on the stored inputs."""
    from oracle import retrieval_ref as rr
    g = np.load(os.path.join(GOLDEN, "itm_eval_small.npz"))
    sim = rr.similarity(g["img_feat"], g["txt_feat"])
    assert np.allclose(sim, g["sim"], rtol=1e-6, atol=1e-6)
    img2txt = [list(r) for r in g["img2txt"]]
    res = rr.itm_eval(sim, sim.T.copy(), g["txt2img"], img2txt)
    want = dict(zip([str(k) for k in g["keys"]], g["values"]))
    assert set(res) == set(want)
    for k in want:
        assert abs(res[k] - want[k]) < 1e-9, (k, res[k], want[k])
    r_i, r_t = rr.ranks(sim, sim.T.copy(), g["txt2img"], img2txt)
    assert (r_i == g["rank_i2t"]).all() and (r_t == g["rank_t2i"]).all()
    # the count form used on the GPU equals the argsort form when there are no ties
    best = np.array([sim[i, img2txt[i]].max() for i in range(sim.shape[0])])
    assert ((sim > best[:, None]).sum(1) == r_i).all()
    ref = sim[g["txt2img"], np.arange(sim.shape[1])]
    assert ((sim > ref[None, :]).sum(0) == r_t).all()


def test_nearest_neighbor_oracle_matches_reference_golden_and_sklearn():
    """tests/golden/nearest_neighbor_small.npz holds the output of the reference's own nearest_neighbor
    (distill.py:89-95).  sklearn (the reference's dependency) is importable here, so the restatement is
    also checked against cosine_similarity directly."""
    from oracle import retrieval_ref as rr
    g = np.load(os.path.join(GOLDEN, "nearest_neighbor_small.npz"))
    sentences = list(range(g["bank"].shape[0]))
    got = rr.nearest_neighbor(sentences, g["query"], g["bank"])
    assert got == g["index"].tolist()
    from sklearn.metrics.pairwise import cosine_similarity
    rng = np.random.RandomState(0)
    bank, query = rng.randn(300, 40), rng.randn(9, 40)
    want = [int(np.argmax(cosine_similarity(q.reshape(1, -1), bank))) for q in query]
    assert rr.nearest_neighbor(list(range(300)), query, bank) == want


def test_bench_algorithmic_flops_match_the_network_spec():
    """bench.py prices an iteration at syn_steps * 9 * 2 * MACs_fwd.  The per-image MAC count it
    uses (4.2419 G for NFNet-l0 at 224x224) is re-derived here from the oracle's layers by running one image
    through forward hooks; the text head's 7.08 M from its two linear layers."""
    import bench
    enc = nr.ImageEncoder("nfnet_l0")
    macs = [0]

    def hook(mod, inp, out):
        w = mod.weight
        macs[0] += out.shape[2] * out.shape[3] * w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3]
    hs = [m.register_forward_hook(hook) for m in enc.modules() if isinstance(m, nr.ScaledStdConv2d)]
    with torch.no_grad():
        enc(torch.zeros(1, 3, 224, 224))
    for h in hs:
        h.remove()
    assert abs(macs[0] - 4.2419e9) / 4.2419e9 < 1e-4, macs[0]
    head = 768 * 2304 + 2304 * 2304
    assert abs(head - 7.08e6) / 7.08e6 < 2e-3
    want = 8 * 9 * 2 * (100 * (macs[0] + head) + 100 * 100 * 2304)
    assert abs(bench.algorithmic_flops_per_iter(100, 8) - want) / want < 1e-3
    assert abs(bench.algorithmic_flops_per_iter(100, 8) - 61.2e12) / 61.2e12 < 2e-3


def test_vit_structural_anchors():
    """oracle/vit_ref.py restates timm 0.6.7's VisionTransformer (parity unpinned: timm is absent).  What CAN be
    checked: the published parameter counts (with timm's 1000-way head) and the flatten order ReparamModule gives."""
    from oracle import vit_ref as vr, distill_ref as dr
    enc = vr.ImageEncoder("vit_b16")
    n = sum(p.numel() for p in enc.parameters())
    assert n == 85_798_656 and n + 768 * 1000 + 1000 == 86_567_656          # vit_base_patch16_224: 86.6 M
    assert enc.model.num_features == 768 and enc.model.num_tokens == 197
    tiny = vr.ImageEncoder("vit_tiny16")
    nt = sum(p.numel() for p in tiny.parameters())
    assert nt + 192 * 1000 + 1000 == 5_717_416                               # vit_tiny_patch16_224: 5.7 M
    # the reference's 'vit' keeps timm's 1000-way head (networks.py:668 passes no num_classes=0): 5,717,416 parameters,
    # registered after `norm`, 1000-d features (networks.py:819)
    cls = vr.ImageEncoder("vit_tiny16_cls")
    assert sum(p.numel() for p in cls.parameters()) == 5_717_416 and cls.model.num_features == 1000
    assert [n for n, _ in cls.named_parameters()][-4:] == ["model.norm.weight", "model.norm.bias", "model.head.weight",
                                                           "model.head.bias"]
    fm = dr.FlatModule(vr.ImageEncoder("vit_micro"))
    assert fm.names[:4] == ["model.cls_token", "model.pos_embed", "model.patch_embed.proj.weight",
                            "model.patch_embed.proj.bias"]
    assert fm.names[4:16] == ["model.blocks.0." + s for s in (
        "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
        "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]
    assert fm.names[-2:] == ["model.norm.weight", "model.norm.bias"]
    x = torch.randn(3, 3, 32, 32)
    assert fm(x, flat_param=fm.flat_param()).shape == (3, 64)


def test_squeeze_excite_gate_from_the_mid_channel_pooled_vector():
    """The identity the engine's SE path rests on: conv3 of a NormFreeBlock is a
    pointwise conv, hence linear, so the pooled conv3 output timm's SEModule starts from (oracle/nfnet_ref.py
    SEModule.forward: `x.mean((2, 3))`) equals conv3's standardised weight applied to the pooled MID-channel
    activation plus its bias -- and the gradient of any function of that pooled vector w.r.t. the mid activation is
    the per-image vector W3^T pb / hw broadcast over the pixels."""
    from oracle import nfnet_ref as nr
    torch.manual_seed(0)
    enc = nr.ImageEncoder("nfnet_tiny")
    nr.randomize_like_trained(enc, 1)
    blk = enc.model.stages[2][0]
    conv3 = blk.conv3
    n, c, h = 3, conv3.in_channels, 5
    a = torch.randn(n, c, h, h, dtype=torch.float64).float().requires_grad_(True)
    y = conv3(a)
    p_ref = y.mean((2, 3))
    w3 = conv3.standardized_weight().reshape(conv3.out_channels, c)
    p_mid = a.mean((2, 3)) @ w3.t() + conv3.bias
    assert torch.allclose(p_ref, p_mid, rtol=1e-5, atol=1e-6)
    pb = torch.randn_like(p_ref)
    ga, = torch.autograd.grad((p_ref * pb).sum(), a)
    want = (pb @ w3 / (h * h))[:, :, None, None].expand_as(a)
    assert torch.allclose(ga, want, rtol=1e-5, atol=1e-7)


def test_goldens_are_present_and_well_formed():
    """Every fixture the GPU suite compares against exists, loads without pickle, and holds finite numbers
    (tests/golden/*.npz are written by oracle/gen_golden.py in the build container: the GPU box never sees the reference)."""
    want = {"unroll_tiny": ["it0_grand", "it1_grand", "theta0_img_sample", "perms"],
            "unroll_c1_scalars": ["it0_grand", "it0_g_image_syn_slice", "it0_g_text_syn"],
            "unroll_c2s_scalars": ["it0_grand", "it0_g_image_syn_slice", "it0_text_syn_after"],
            "unroll_k8_scalars": ["it0_grand", "it0_ces", "it0_g_image_syn_slice", "it0_text_syn_after", "perms"],
            "text_only_unroll": ["grand", "g_text_syn", "theta0_sample"], "itm_eval_small": ["rank_i2t"],
            "nearest_neighbor_small": ["index"], "reparam_reference": ["head_y", "toy_y", "toy_g_theta"]}
    for name, keys in want.items():
        g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        for k in keys:
            assert k in g.files, (name, k)
            if g[k].dtype.kind == "f":
                assert np.isfinite(g[k]).all(), (name, k)
    k8 = np.load(os.path.join(GOLDEN, "unroll_k8_scalars.npz"))
    assert (int(k8["n"]), int(k8["K"]), int(k8["size"]), str(k8["variant"])) == (12, 8, 224, "nfnet_l0")
    assert k8["perms"].shape == (1, 8, 12) and k8["it0_ces"].shape == (8,) and 0.5 < float(k8["it0_grand"]) < 50
