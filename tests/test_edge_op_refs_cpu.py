"""The float64 references of tests/edge_op_refs.py, checked without a GPU: against independent formulations (1e-12) and
the repository's oracles, the properties claimed beside each shape, that each plausible kernel mistake moves the affected
output by at least ten times the cap tests/test_gpu_edge_ops.py holds the kernels to, and the host-side refusals of the
op-level entry points (mdd_op_image_edge, mdd_op_vit_glue, mdd_op_lin_pack, mdd_op_resid, mdd_flat_*)."""
import pytest
import torch
import torch.nn.functional as F

import edge_op_refs as R

CAP_F32, CAP_BF16 = 3e-6, 5e-3          # tests/test_gpu_edge_ops.py
TOL = 1e-12


def close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a.double() - b.double()).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def far(wrong, ref, cap, rows=lambda t: t):
    e = R.row_err(rows(wrong), rows(ref))
    assert e >= 10 * cap, (e, cap)


def cap_of(dtype):
    return CAP_F32 if dtype == "f32" else CAP_BF16


# ------------------------------------------------------------------------------------------------ independent formulations
@pytest.mark.parametrize("s,cout,dtype", R.stem_cases())
def test_stem_dgrad_reference_matches_conv_transpose_and_the_tap_formula(s, cout, dtype):
    i = R.stem_inputs(s, cout, dtype)
    for dy, w in ((i["dy1"], i["w1"]), (i["dy2"], i["w2"])):
        g = R.stem_dgrad(dy, w, s)
        close(F.conv_transpose2d(dy.double(), w.double(), None, 2, 1, output_padding=1), g)
        close(R.stem_dgrad_taps(dy, w, s), g)


def test_stem_dgrad_reference_matches_the_oracle_stem_convolution():
    """oracle/nfnet_ref.ScaledStdConv2d(3, cout, 3, stride 2) is the layer: its input gradient, with its standardised
    weight, is the reference's"""
    from oracle import nfnet_ref as nr
    torch.manual_seed(3)
    conv = nr.ScaledStdConv2d(3, 16, 3, stride=2, gamma=nr.GAMMA_SILU).double()
    x = torch.randn(2, 3, 24, 24, dtype=R.F64, requires_grad=True)
    y = conv(x)
    dy = torch.randn_like(y)
    (g,) = torch.autograd.grad(y, x, dy)
    close(R.stem_dgrad(dy, conv.standardized_weight().detach(), 24), g)


@pytest.mark.parametrize("s,p", R.PATCH_SP)
def test_patchify_reference_is_the_patch_embedding(s, p):
    i = R.patch_inputs(s, p, "f32")
    cols = R.patchify_ref(i["image"], R.IDX, p)
    close(R.patchify_index(i["image"], R.IDX, p), cols)
    D = 24
    w, b = torch.randn(D, 3, p, p, generator=R._gen(1, s, p)).double(), torch.randn(D, generator=R._gen(2, s, p)).double()
    emb = F.conv2d(i["image"][R.IDX].double(), w, b, stride=p).flatten(2).transpose(1, 2).reshape(-1, D)
    close(cols @ w.view(D, -1).t() + b, emb)
    # its backward: the adjoint map
    cb = R.patch_inputs(s, p, "f32")["colsbar"].double()
    img = i["image"][R.IDX].double().requires_grad_(True)
    (g,) = torch.autograd.grad(R.patchify_index(img, None, p), img, cb)
    ref = R.unpatchify_ref(i["dimage0"], cb, R.IDX, R.COEF, R.MUL, s, p)
    close(R.scatter_rows(i["dimage0"], R.IDX, R.factor(R.COEF, R.MUL) * g), ref)


def test_patchify_and_embed_references_match_the_oracle_vit():
    """oracle/vit_ref: patch embedding = patchify x the flattened Conv2d weight, and the token assembly"""
    from oracle import vit_ref as vr
    s, p, dim = 16, 8, 64
    torch.manual_seed(5)
    m = vr.VisionTransformer(vr.VitCfg(img_size=s, patch=p, dim=dim, depth=1, heads=2)).double()
    vr.randomize_like_trained(m, 7)
    img = R.patch_inputs(s, p, "f32")["image"].double()
    seen = {}
    h = m.blocks.register_forward_pre_hook(lambda mod, args: seen.update(x0=args[0].detach().clone()))     # returns None
    m(img[R.IDX])
    h.remove()
    pe = R.patchify_ref(img, R.IDX, p) @ m.patch_embed.proj.weight.detach().view(dim, -1).t() + m.patch_embed.proj.bias.detach()
    close(pe.view(R.N, -1, dim), m.patch_embed(img[R.IDX]).detach())
    close(R.embed(pe.view(R.N, -1, dim), m.cls_token.detach().view(dim), m.pos_embed.detach()[0]), seen["x0"])


@pytest.mark.parametrize("case", R.IM2COL)
def test_im2col_reference_times_the_packed_weight_is_the_convolution(case):
    h, w, k, stride, pad, cpad = case
    x = R.im2col_input(case, "bf16")
    col = R.im2col_ref(x, k, stride, pad)
    close(R.im2col_index(x, k, stride, pad), col)
    cout = 5
    wgt = torch.randn(cout, cpad, k, k, generator=R._gen(3, *case)).double()
    y = F.conv2d(x.double().permute(0, 3, 1, 2), wgt, None, stride, pad)
    close(col @ R.pack_fwd(wgt).view(cout, -1).t(), y.permute(0, 2, 3, 1).reshape(-1, cout))
    assert col.shape == (R.IM2COL_N * y.shape[2] * y.shape[3], k * k * cpad) and y.shape[2:] == R.im2col_out(h, w, k, stride, pad)


@pytest.mark.parametrize("n,tok,dim", R.GLUE)
def test_glue_references_match_autograd(n, tok, dim):
    i = {k: v.double() for k, v in R.glue_inputs(n, tok, dim, "f32").items()}
    x0 = R.embed(i["pe"], i["cls"], i["pos"])
    assert x0.shape == (n, tok, dim)
    close(x0[:, 0], (i["cls"] + i["pos"][0]).expand(n, dim)), close(x0[:, 1:], i["pe"] + i["pos"][1:])
    eps = 1e-6           # the map is linear: a finite difference is exact up to rounding
    fd = (R.embed(i["pe"] + eps * i["pe_t"], i["cls"] + eps * i["cls_t"], i["pos"] + eps * i["pos_t"]) - x0) / eps
    assert float((fd - R.embed_tangent(i["pe"], i["pe_t"], i["cls"], i["cls_t"], i["pos"], i["pos_t"])).abs().max()) < 1e-8
    pe, cls, pos = (i[k].clone().requires_grad_(True) for k in ("pe", "cls", "pos"))
    g = torch.autograd.grad(R.embed(pe, cls, pos), (pe, pos, cls), i["xb"])
    for got, ref in zip(R.embed_bwd(i["xb"]), (g[0], g[1], g[2].view(1, dim))):
        close(got, ref)
    c = i["c"]
    close(R.cls_gather(R.cls_scatter(c, tok)), c)
    assert float(R.cls_scatter(c, tok)[:, 1:].abs().max()) == 0.0


def test_resid_reference_matches_the_oracle_block():
    """oracle/nfnet_ref.NormFreeBlock: out * alpha + shortcut, and the next block's F.silu(x) * beta"""
    from oracle import nfnet_ref as nr
    torch.manual_seed(0)
    enc = nr.ImageEncoder("nfnet_tiny")
    nr.randomize_like_trained(enc, 1)
    net = enc.model.double()
    blk, nxt = net.stages[1][1], net.stages[2][0]
    assert blk.downsample is None
    seen = {}
    keep = lambda **kw: seen.update({k: v.detach().clone() for k, v in kw.items()})       # returns None: a hook's value would replace the tensor
    hooks = [blk.register_forward_pre_hook(lambda m, a: keep(sc=a[0])),
             blk.attn_last.register_forward_hook(lambda m, a, out: keep(c3=blk.attn_gain * out)),
             nxt.conv1.register_forward_pre_hook(lambda m, a: keep(a=a[0])),
             nxt.register_forward_pre_hook(lambda m, a: keep(x=a[0]))]
    net(torch.randn(2, 3, 64, 64, dtype=R.F64, generator=R._gen(9)))
    for h in hooks:
        h.remove()
    assert float(seen["c3"].abs().max()) > 1e-3
    x, a = R.resid(seen["c3"], seen["sc"], "silu", alpha=blk.alpha, beta=nxt.beta)
    close(x, seen["x"]), close(a, seen["a"])


@pytest.mark.parametrize("act", ["relu", "silu"])
def test_resid_references_match_their_closed_forms(act):
    i = {k: v.double() for k, v in R.resid_inputs(4104, "bf16").items()}
    x, a = R.resid(i["c3"], i["sc"], act)
    x_t, a_t = R.resid_tangent(i["c3"], i["c3_t"], i["sc"], i["sc_t"], act)
    close(x, R.ALPHA * i["c3"] + i["sc"]), close(x_t, R.ALPHA * i["c3_t"] + i["sc_t"])
    sg = torch.sigmoid(x)
    d = (x > 0).double() if act == "relu" else sg * (1 + x * (1 - sg))
    close(a, R.BETA * (x.clamp(min=0) if act == "relu" else x * sg)), close(a_t, R.BETA * d * x_t)


def test_flat_references():
    i = R.flat_inputs(1027)
    lam = R.lambda_init(i["a"], i["b"], i["dist0"])
    d = ((i["a"].double() - i["b"].double()) ** 2).sum() / i["dist0"]
    a = i["a"].double().requires_grad_(True)
    (g,) = torch.autograd.grad(((a - i["b"].double()) ** 2).sum() / i["dist0"][0], a)       # d (dist / dist0) / d theta_K
    close(lam, g)
    m = R.match_finalize(i["s4"])
    assert float(m[0]) == float(i["s4"][0] / i["s4"][1] + i["s4"][2] / i["s4"][3]) and d > 0
    # the dot product's inputs do not cancel: |<a, b>| is a fair denominator at every n
    for n in R.FLAT_N:
        j = R.flat_inputs(n)
        dot = float(j["a"].double() @ j["b"].double())
        assert abs(dot) >= 0.1 * float(j["a"].double().norm() * j["b"].double().norm()), n


# ------------------------------------------------------------------------------------------------ what the shapes reach
def test_shapes_reach_the_paths_claimed_beside_them():
    # stem dgrad: row blocks, spans
    assert [R.stem_plan(s) for s in R.STEM_S] == [(1, 1, 1), (3, 1, 3), (17, 2, 34)]
    assert all(s % 8 == 0 for s in R.STEM_S) and 136 // 2 > 64 and 136 - 128 == 8
    assert len(set(R.IDX.tolist())) == R.N and R.IDX.tolist() != sorted(R.IDX.tolist()) and int(R.IDX.max()) < R.NQ
    assert R.factor(R.COEF, R.MUL) == R.COEF * R.MUL
    # gather / scatter: a ragged last block, h != w
    assert all((R.N * h * w) % 256 != 0 for h, w in R.GS_HW) and any(h != w for h, w in R.GS_HW)
    assert [-(-R.N * h * w // 256) for h, w in R.GS_HW] == [1, 7, 1]
    assert all(s % p == 0 for s, p in R.PATCH_SP)
    # im2col: items per output row against the 256 threads of a block
    assert [R.im2col_out(*c[:5]) for c in R.IM2COL] == [(7, 5), (8, 8), (10, 10)]
    assert [R.im2col_out(*c[:5])[1] * c[2] ** 2 * (c[5] // 8) for c in R.IM2COL] == [245, 392, 90]
    # linear packing: offsets, tiles (the engine's formula: ceil(in / 64) * ceil(out / 64) per layer), parities
    for launch, shapes in R.LP_LAUNCHES.items():
        descs, tiles, nth, npk = R.lp_descs(shapes)
        assert tiles == sum(-(-o // 64) * -(-i // 64) for o, i in shapes)
        assert nth == sum(o * i + o for o, i in shapes) == R.lp_theta(launch).numel() and npk == sum(o * i for o, i in shapes)
        assert [d[4] for d in descs] == [sum(-(-o // 64) * -(-i // 64) for o, i in shapes[:j]) for j in range(len(shapes))]
    assert R.lp_descs(R.LP_LAUNCHES["vit"])[1] == 3 + 1 + 4 + 4 + 2 + 4
    assert all(R.lp_paired(d) == (True, True) for d in R.lp_descs(R.LP_LAUNCHES["vit"])[0])
    odd = R.lp_descs(R.LP_LAUNCHES["odd"])[0]
    assert [(d[0] % 2, d[1] % 2) for d in odd] == [(0, 0), (0, 1), (0, 0)] and [d[1] for d in odd] == [0, 231, 276]
    assert [R.lp_paired(d) for d in odd] == [(False, False), (False, False), (True, True)]
    off = R.lp_descs(R.LP_LAUNCHES["odd_offset"])[0]
    assert off[1][1] == 15 and off[1][2:4] == (64, 64) and R.lp_paired(off[1]) == (False, False)
    # residual sums: trips of the grid-stride loop
    assert [R.resid_trips(e, "bf16") for e in R.RESID_ELEMS] == [1, 1, 2]
    assert R.resid_trips(R.RESID_ELEMS[2] - 8, "bf16") == 1 and R.resid_trips(R.RESID_ELEMS[2], "f32") == 3
    assert all(e % 8 == 0 for e in R.RESID_ELEMS)
    # flat: float4 items and tails
    assert [(n >> 2, n & 3) for n in R.FLAT_N] == [(0, 1), (0, 3), (1, 0), (256, 3), (2048 * 256 + 1, 1)]


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("elems", R.RESID_ELEMS)
def test_resid_inputs_stay_clear_of_the_relu_kink(elems, dtype):
    i = R.resid_inputs(elems, dtype)
    x, _ = R.resid(i["c3"], i["sc"], "relu")
    assert float(x.abs().min()) > R.RESID_CLEAR
    assert 0.3 < float((x > 0).double().mean()) < 0.7


# ------------------------------------------------------------------------------------------------ planted mistakes
@pytest.mark.parametrize("s,cout,dtype", R.stem_cases())
def test_stem_inputs_expose_wrong_kernels(s, cout, dtype):
    i = R.stem_inputs(s, cout, dtype)
    ref = R.stem_ref(s, cout, dtype, True, R.IDX, R.COEF, R.MUL)
    rows = R.image_rows
    wrong = lambda **kw: R.stem_ref(s, cout, dtype, True, R.IDX, R.COEF, R.MUL, grad=lambda dy, w, s_: R.stem_dgrad_taps(dy, w, s_, **kw))
    far(wrong(swap_tx=True), ref, CAP_F32, rows)
    far(wrong(clamp_rows=True), ref, CAP_F32, rows)
    if s > 128:
        far(wrong(drop_col64=True), ref, CAP_F32, rows)
    else:
        close(wrong(drop_col64=True), ref)            # no seam at this size
    far(R.stem_ref(s, cout, dtype, False, R.IDX, R.COEF, R.MUL), ref, CAP_F32, rows)       # the second source dropped
    far(R.stem_ref(s, cout, dtype, True, R.IDX, None, R.MUL), ref, CAP_F32, rows)          # coef ignored
    far(R.stem_ref(s, cout, dtype, True, None, R.COEF, R.MUL), ref, CAP_F32, rows)         # idx taken as the identity
    # a padded weight lane read in the place of channel 2
    wt = R.stem_wt(i["w1"])
    assert bool((wt[3:] == R.GARBAGE).all()) and torch.equal(wt[:3, 4], i["w1"][:, :, 1, 1].t())
    w_bad = i["w1"].clone()
    w_bad[:, 2] = wt[3].view(3, 3, cout).permute(2, 0, 1)
    g = R.stem_dgrad(i["dy1"], w_bad, s) + R.stem_dgrad(i["dy2"], i["w2"], s)
    far(R.scatter_rows(i["dimage0"], R.IDX, R.factor(R.COEF, R.MUL) * g), ref, CAP_F32, rows)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_edge_inputs_expose_wrong_kernels(dtype):
    for h, w in R.GS_HW:
        i = R.gs_inputs(h, w, dtype)
        ref = R.scatter_ref(i["dimage0"], i["x0bar"], R.IDX, R.COEF, R.MUL)
        shifted = i["x0bar"].roll(-1, 3)                # channel c + 1 read: the last real channel takes a padded lane
        far(R.scatter_ref(i["dimage0"], shifted, R.IDX, R.COEF, R.MUL), ref, CAP_F32, R.image_rows)
        far(R.scatter_ref(i["dimage0"], i["x0bar"], None, R.COEF, R.MUL), ref, CAP_F32, R.image_rows)
    for case in R.IM2COL:
        x = R.im2col_input(case, dtype)
        _, _, k, stride, pad, _ = case
        ref = R.im2col_ref(x, k, stride, pad)
        far(R.im2col_index(x, k, stride, pad, tx_major=True), ref, cap_of(dtype))
        far(R.im2col_index(x, k, stride, pad, pad_used=pad - 1), ref, cap_of(dtype))
    for s, p in R.PATCH_SP:
        i = R.patch_inputs(s, p, dtype)
        far(R.patchify_index(i["image"], R.IDX, p, swap=True), R.patchify_ref(i["image"], R.IDX, p), cap_of(dtype))


def test_lin_pack_inputs_expose_wrong_kernels():
    shapes = R.LP_LAUNCHES["vit"]
    (wf, wt), (wf_t, wt_t) = R.lp_refs("vit"), R.lp_refs("vit", tangent=True)
    assert not bool(torch.isnan(torch.cat([wf, wt, wf_t, wt_t])).any())          # the NaN biases are not in the packing
    li = shapes.index((72, 40))
    bad = R.lp_rows(R.lp_refs("vit", untransposed_tile=True)[1], shapes, "wt")[li]
    far(bad, R.lp_rows(wt, shapes, "wt")[li], CAP_BF16)
    for a, b in zip(R.lp_rows(wf, shapes, "wf"), R.lp_rows(wf_t, shapes, "wf")):    # the tangent written from the primal
        far(a, b, CAP_BF16)
    w = R.lp_theta("vit")[:192 * 64].view(192, 64).double()
    close(R.lp_rows(wf, shapes, "wf")[0], w), close(R.lp_rows(wt, shapes, "wt")[0], w.t())


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("n,tok,dim", R.GLUE)
def test_glue_inputs_expose_wrong_kernels(n, tok, dim, dtype):
    i, cap = R.glue_inputs(n, tok, dim, dtype), cap_of(dtype)
    tokens = lambda t: t.reshape(-1, dim)
    ref = R.embed(i["pe"], i["cls"], i["pos"])
    far(R.embed(i["pe"], i["cls"], i["pos"], pos_shift=True), ref, cap, tokens)
    far(R.embed(i["pe"], i["cls"], i["pos"], cls_everywhere=True), ref, cap, tokens)
    _, dpos, dcls = R.embed_bwd(i["xb"])
    if n > 1:
        far(R.embed_bwd(i["xb"], dpos_last_only=True)[1], dpos, CAP_F32)
    far(R.embed_bwd(i["xb"], dcls_token1=True)[2], dcls, CAP_F32)
    # a tangent call that returns the primal sums
    far(dpos, R.embed_bwd(i["xb_t"])[1], CAP_F32)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_resid_and_flat_inputs_expose_wrong_kernels(dtype):
    i, cap = R.resid_inputs(4104, dtype), cap_of(dtype)
    x_t, a_t = R.resid_tangent(i["c3"], i["c3_t"], i["sc"], i["sc_t"], "relu")
    far(R.resid_tangent(i["c3"], i["c3_t"], i["sc"], i["sc_t"], "relu", own_sign=True)[1], a_t, cap, R.flat_rows)
    for act in ("relu", "silu"):
        x, a = R.resid(i["c3"], i["sc"], act)
        xw, aw = R.resid(i["c3"], i["sc"], act, alpha_on_shortcut=True)
        far(xw, x, cap, R.flat_rows), far(aw, a, cap, R.flat_rows)
    j = R.flat_inputs(1027)
    lam = R.lambda_init(j["a"], j["b"], j["dist0"])
    far(R.lambda_init(j["a"], j["b"], j["dist0"], two=1.0).view(-1, 1), lam.view(-1, 1), CAP_F32)


# ------------------------------------------------------------------------------------------------ host-side refusals
def test_entry_points_reject_bad_arguments_before_any_launch():
    """mdd_op_image_edge / mdd_op_vit_glue / mdd_op_lin_pack / mdd_op_resid / mdd_flat_* validate on the host: none of these
    calls reaches a kernel (no GPU needed)."""
    import ctypes as C
    import os
    from multimodal_dataset_distillation_amd import _lib, build_ext
    if not os.path.exists(_lib.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _lib.load()
    p = C.c_void_p(64)      # never dereferenced: every call below fails its argument check
    err = lambda: lib.mdd_last_error()

    def edge(op, dtype=0, n=3, h=8, w=8, c=8, k=0, stride=0, pad=0, image=None, idx=None, coef=None, a=None, wt1=None, a2=None,
             wt2=None, out=None, dimage=None):
        return lib.mdd_op_image_edge(dtype, op, n, h, w, c, k, stride, pad, 1.0, image, idx, coef, a, wt1, a2, wt2, out, dimage, None)
    assert edge(6, image=p, out=p) == 2 and b"invalid argument" in err() and edge(-1, image=p, out=p) == 2
    assert edge(0, dtype=2, image=p, out=p) == 2 and edge(0, n=0, image=p, out=p) == 2
    assert edge(0, out=p) == 2 and edge(0, image=p) == 2 and edge(0, image=p, out=p, a=p) == 2 and edge(0, image=p, out=p, coef=p) == 2
    assert edge(0, image=p, out=p, c=2) == 2 and edge(0, image=p, out=p, k=3) == 2 and edge(0, image=p, out=p, wt1=p) == 2
    assert edge(1, dimage=p) == 2 and edge(1, a=p) == 2 and edge(1, a=p, dimage=p, out=p) == 2 and edge(1, a=p, dimage=p, c=2) == 2
    assert edge(2, a=p, dimage=p) == 2 and edge(2, a=p, wt1=p, dimage=p, a2=p) == 2 and edge(2, a=p, wt1=p, dimage=p, wt2=p) == 2
    assert edge(2, a=p, wt1=p, dimage=p, h=8, w=16) == 2
    assert edge(2, a=p, wt1=p, dimage=p, h=12, w=12) == 2 and b"multiple of 8" in err()        # launch_stem_dgrad_image says no
    assert edge(2, a=p, wt1=p, dimage=p, c=32) == 2 and b"cout 8 or 16" in err()
    assert edge(3, image=p, out=p, c=3, h=24, w=24, k=16) == 2 and b"s % p" in err()
    assert edge(3, image=p, out=p, c=3, h=16, w=24, k=8) == 2 and edge(3, image=p, out=p, c=3, h=16, w=16, k=0) == 2
    assert edge(4, a=p, dimage=p, c=3, h=24, w=24, k=16) == 2 and edge(4, a=p, out=p, c=3, h=16, w=16, k=8) == 2
    assert edge(5, a=p, out=p, k=7, stride=0, pad=3) == 2 and edge(5, a=p, out=p, k=7, stride=2, pad=-1) == 2
    assert edge(5, a=p, out=p, k=7, stride=2, pad=3, c=6) == 2 and b"16-byte chunk" in err()
    assert edge(5, dtype=1, a=p, out=p, k=7, stride=2, pad=3, c=12) == 2 and edge(5, a=p, out=p, k=7, stride=2, pad=3, idx=p) == 2
    assert edge(5, a=p, out=p, k=20, stride=1, pad=1) == 2

    def glue(op, dtype=0, n=2, tok=5, dim=8, a=p, a_t=None, b=None, b_t=None, cls=None, cls_t=None, pos=None, pos_t=None, out=p,
             out_t=None, dcls=None, dpos=None):
        return lib.mdd_op_vit_glue(dtype, op, n, tok, dim, a, a_t, b, b_t, cls, cls_t, pos, pos_t, out, out_t, dcls, dpos, None)
    assert glue(7) == 2 and b"invalid argument" in err() and glue(-1) == 2 and glue(2, dtype=3) == 2 and glue(2, tok=0) == 2
    assert glue(2, a=None) == 2 and glue(2, out=None) == 2 and glue(2, a_t=p, out_t=p) == 2 and glue(5, a_t=p) == 2
    assert glue(0) == 2 and glue(0, cls=p) == 2 and glue(0, cls=p, pos=p, cls_t=p) == 2
    assert glue(0, cls=p, pos=p, a_t=p, out_t=p, cls_t=p) == 2 and glue(0, cls=p, pos=p, a_t=p, cls_t=p, pos_t=p) == 2
    assert glue(0, cls=p, pos=p, tok=1) == 2 and glue(0, cls=p, pos=p, dcls=p) == 2
    assert glue(1) == 2 and glue(1, dcls=p) == 2 and glue(1, dcls=p, dpos=p, a_t=p) == 2 and glue(1, dcls=p, dpos=p, cls=p) == 2
    assert glue(2, b=p) == 2 and glue(3, pos=p) == 2 and glue(4) == 2 and glue(4, b=p, a_t=p, out_t=p) == 2
    assert glue(4, b=p, n=1, tok=3, dim=2) == 2 and b"16-byte chunk" in err() and glue(4, dtype=1, b=p, n=1, tok=3, dim=4) == 2

    shapes = lambda *rows: (C.c_int32 * (2 * len(rows)))(*[v for r in rows for v in r])
    ok = shapes((64, 64))
    lp = lambda dtype=0, n=1, sh=ok, th=p, th_t=None, wf=p, wt=p, wf_t=None, wt_t=None: \
        lib.mdd_op_lin_pack(dtype, n, sh, th, th_t, wf, wt, wf_t, wt_t, None)
    assert lp(dtype=2) == 2 and b"invalid argument" in err() and lp(n=0) == 2 and lp(sh=None) == 2 and lp(th=None) == 2
    assert lp(wf=None) == 2 and lp(wt=None) == 2 and lp(wf_t=p) == 2 and lp(th_t=p) == 2 and lp(th_t=p, wf_t=p) == 2
    assert lp(sh=shapes((0, 64))) == 2 and lp(n=2, sh=shapes((64, 64), (8, -1))) == 2

    rs = lambda op, dtype=0, elems=8, c3=p, c3_t=None, sc=p, sc_t=None, xo=p, xo_t=None, ao=None, ao_t=None: \
        lib.mdd_op_resid(dtype, op, elems, 0.2, 1.0, c3, c3_t, sc, sc_t, xo, xo_t, ao, ao_t, None)
    assert rs(3) == 2 and b"invalid argument" in err() and rs(-1) == 2 and rs(0, dtype=2) == 2
    assert rs(0, elems=0) == 2 and rs(0, elems=6) == 2 and b"16-byte chunk" in err() and rs(1, dtype=1, elems=12) == 2
    assert rs(0, c3=None) == 2 and rs(0, sc=None) == 2 and rs(1, xo=None) == 2
    assert rs(0, c3_t=p) == 2 and rs(0, c3_t=p, sc_t=p) == 2 and rs(1, sc_t=p) == 2 and rs(1, xo_t=p) == 2
    assert rs(0, ao_t=p) == 2 and rs(1, c3_t=p, sc_t=p, xo_t=p, ao_t=p) == 2         # ao_t: tangent form, with the stashed ao
    assert rs(2) == 2 and rs(2, sc=None, ao=p) == 2 and rs(2, sc=None, c3_t=p) == 2

    assert lib.mdd_flat_dot(None, p, p, 1.0, 4, None) == 2 and b"invalid argument" in err()
    assert lib.mdd_flat_dot(p, p, None, 1.0, 4, None) == 2 and lib.mdd_flat_dot(p, p, p, 1.0, -1, None) == 2
    assert lib.mdd_flat_scale_out(None, p, None, 1.0, 4, None) == 2 and lib.mdd_flat_scale_out(p, None, None, 1.0, 4, None) == 2
    assert lib.mdd_flat_sub_inplace(p, None, 4, None) == 2 and lib.mdd_flat_sub_inplace(p, p, -4, None) == 2
    assert lib.mdd_flat_lambda_init(p, p, p, None, 4, None) == 2 and lib.mdd_flat_lambda_init(None, p, p, p, 4, None) == 2
    assert lib.mdd_flat_match_finalize(None, p, None) == 2 and lib.mdd_flat_match_finalize(p, None, None) == 2
    assert lib.mdd_flat_d2f(p, None, 1.0, 0, 1, None) == 2 and lib.mdd_flat_d2f(p, p, 1.0, 0, 0, None) == 2
    assert lib.mdd_flat_d2f(p, p, 1.0, 0, 65, None) == 2 and b"64 scalars" in err()
    assert lib.mdd_flat_accum_f2d(None, p, 1.0, None) == 2 and lib.mdd_flat_accum_f2d(p, None, 1.0, None) == 2
