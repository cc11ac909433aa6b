"""The kernels at the edges of every pass -- k_img_gather, k_img_scatter, k_stem_dgrad_image<AT, 8 | 16> (csrc/elementwise.hip),
k_patchify, k_unpatchify_accum (csrc/vit.hip), k_im2col (csrc/nfres.hip) --, the ViT's packing and token glue
(k_lin_pack_all, k_vit_embed / k_vit_embed_bwd / k_add2 as float and as Dual, k_cls_gather, k_cls_scatter, k_act_to_f32,
k_f32_to_act), the residual sums without squeeze-excite (k_resid_relu / k_resid_silu as float and as Dual, k_scale) and the
reverse sweep's flat kernels (k_dot, k_scale_out, k_sub_inplace, k_lambda_init, k_match_finalize, k_d2f, k_accum_f2d:
csrc/flat_ops.hip), each in fp32 and bf16 storage where it has a storage type, at the op level (mdd_op_image_edge,
mdd_op_vit_glue, mdd_op_lin_pack, mdd_op_resid, mdd_flat_*) against the float64 references of tests/edge_op_refs.py,
evaluated on the same storage-rounded inputs.

The error of a tensor is the MAXIMUM OVER ROWS of the row's norm-relative error: a row is one (image, channel, y) line of
an image gradient, a matrix row of a column / patch matrix, an output channel of wf or an input channel of wt, a token
position, one 8-element chunk of a flat activation tensor, one element of a flat parameter stream.  Pure copies (gather,
patchify, im2col, cls_gather, cls_scatter, act_to_f32, f32_to_act, the patch gradients of embed_bwd, lin_pack) must be
BIT-EQUAL to the reference -- in bf16 storage to torch's .bfloat16(), both round to nearest even -- and their zero lanes +0.
Every output is a slice of a larger allocation with 64 sentinel elements on either side, which must come back
bit-identical, and starts as NaN (an accumulate target: as the random values the reference adds to); every input, in
tangent calls every primal output, and every row of dimage that idx does not name must come back bit-identical.  The
accumulating kernels add without atomics on the engine's guarantee that the rows of idx are distinct within a step: only
distinct rows are tested.  tests/test_edge_op_refs_cpu.py shows that with these inputs each plausible kernel mistake
moves the affected output by at least ten times the caps below."""
import ctypes as C

import pytest
import torch

import edge_op_refs as R
from test_gpu_small_ops import Case, Guarded, P, _lib, _stream, dev

pytestmark = pytest.mark.gpu
DT = {"f32": 0, "bf16": 1}

# Caps, from the project: fp32 outputs 3e-6, tensors stored in bf16 5e-3 (tests/test_gpu_small_ops.py); the dot product
# 1e-6 relative to the float64 dot product of the same fp32 inputs (tests/test_gpu_ops.py test_flat_ops).
CAP_F32, CAP_BF16, CAP_DOT = 3e-6, 5e-3, 1e-6
# Guards per quantity: about twice the largest value measured on MI355X over all cases of this file (each test writes
# every figure to the test report, "edge-ops ..." lines), never above the cap.  Measured maxima:
#   image gradients (fp32, either storage)   stem dgrad 3.6e-7 (s 24, cout 16, fp32 storage; bf16 storage 1.5e-7)
#                                             scatter 5.2e-8   unpatchify_accum 4.6e-8
#   copies, bf16 storage against the UNROUNDED float64 values (fp32 storage: bit-equal, nothing to measure)
#                                             gather 2.2e-3  patchify 1.9e-3  lin_pack 2.9e-3 (a 5-element row)  f32_to_act 2.3e-3
#   token glue   fp32 storage   embed 3.6e-8 / tangent 3.7e-8   add2 3.9e-8 / 3.4e-8
#                bf16 storage   embed 2.2e-3 / 2.4e-3           add2 2.3e-3 / 2.4e-3
#                fp32 sums      dpos 4.4e-8  dcls 3.5e-8  dpos_t 3.8e-8  dcls_t 3.4e-8   (bf16 storage: exact, 0)
#   residual sums, rows of 8   fp32 storage   x' 5.6e-8  a' 2.2e-7 (SiLU; ReLU 1.1e-7)  x'_t 5.6e-8  a'_t 4.2e-7 (SiLU; ReLU 1.1e-7)
#                                             scale 5.5e-8
#                              bf16 storage   x' 3.8e-3  a' 3.9e-3  x'_t 3.8e-3  a'_t 3.9e-3  scale 3.1e-3
#   flat   dot 4.6e-8 (n = 4; 2.4e-11 at n = 2097157)   scale_out 6.0e-8   sub_inplace 6.0e-8   lambda_init 1.6e-7
#          match_finalize 2.5e-8   d2f 1.0e-7   accum_f2d exact
# bf16 storage: the one rounding of the stored value is all there is.  Over a row of 8 elements (the residual sums, 2 M
# rows) the worst row comes close to the format's bound of 2^-8 = 3.9e-3 per element, and twice that is above the cap: those
# guards, and lin_pack's (rows of 5 and 7 elements), ARE the cap.  Where the measured value is 0 or a single fp32 rounding
# the guard is one fp32 rounding (6e-8) rather than twice zero.
_S = lambda f32, bf16: {"f32": f32, "bf16": bf16}
GUARD = {
    "stem_dgrad": 7.1e-7, "scatter": 1.1e-7, "unpatchify": 9.3e-8,
    "gather_round": 4.5e-3, "patchify_round": 3.9e-3, "lp_round": CAP_BF16, "f32_to_act_round": 4.6e-3,
    "embed": _S(7.3e-8, 4.5e-3), "embed_t": _S(7.5e-8, 4.8e-3), "dpos": 9e-8, "dcls": 7e-8, "dpos_t": 7.7e-8, "dcls_t": 6.8e-8,
    "add2": _S(7.9e-8, 4.6e-3), "add2_t": _S(6.9e-8, 4.9e-3),
    "resid_x": _S(1.2e-7, CAP_BF16), "resid_a": _S(4.4e-7, CAP_BF16), "resid_x_t": _S(1.2e-7, CAP_BF16),
    "resid_a_t": _S(8.5e-7, CAP_BF16), "scale": _S(1.1e-7, CAP_BF16),
    "dot": 9.3e-8, "scale_out": 1.2e-7, "sub_inplace": 1.2e-7, "lambda_init": 3.2e-7, "match_finalize": 6e-8,
    "d2f": 2.1e-7, "accum_f2d": 6e-8,
}
BF16_ONLY = ("gather_round", "patchify_round", "lp_round", "f32_to_act_round")     # fp32 storage: bit-equal, nothing to measure


def _guard(kind, dtype):
    g = GUARD[kind]
    return g[dtype] if isinstance(g, dict) else g


def _cap(kind, dtype):
    if kind == "dot":
        return CAP_DOT
    return CAP_BF16 if kind in BF16_ONLY or (isinstance(GUARD[kind], dict) and dtype == "bf16") else CAP_F32


assert all(_guard(k, d) <= _cap(k, d) for k in GUARD for d in R.DTYPES)


class ECase(Case):
    """Case with the row error over a view chosen per comparison, and this file's guards and report prefix"""

    def cmp(self, kind, name, got, ref, rows=lambda t: t):
        torch.cuda.synchronize()
        got.check_sentinels(name)
        assert tuple(got.t.shape) == tuple(ref.shape), (name, got.t.shape, ref.shape)
        self.add(kind, name, R.row_err(rows(got.t.cpu()), rows(ref)))

    def add(self, kind, name, e):
        self.errs.append((kind, name, e))

    def finish(self, report):
        worst = {}
        for k, n, v in self.errs:
            if k not in worst or not v <= worst[k][1]:
                worst[k] = (n, v)
        report(f"edge-ops {self.title}: " + " ".join(f"{k}:{n}={v:.2e}" for k, (n, v) in worst.items()))
        for k, (n, v) in worst.items():
            assert v < _guard(k, self.dtype), (self.title, k, n, v, _guard(k, self.dtype))


def inp(t, dtype=torch.float32):
    """an input on the device, between sentinels, to be checked untouched"""
    return Guarded(tuple(t.shape), dtype, init=t)


def _check(rc):
    from multimodal_dataset_distillation_amd._lib import check
    check(rc)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bits(got, ref, name):
    """got (a Guarded output) is bit-equal to ref (a CPU tensor of the same type): values, the sign of zeros, no NaN left"""
    torch.cuda.synchronize()
    got.check_sentinels(name)
    out = got.t.cpu()
    assert out.dtype == ref.dtype and tuple(out.shape) == tuple(ref.shape), (name, out.dtype, ref.dtype, out.shape, ref.shape)
    assert torch.equal(bits(out), bits(ref)), f"{name}: not bit-equal to the reference"


def assert_other_rows_untouched(g, init, sel, name):
    torch.cuda.synchronize()
    keep = torch.ones(init.shape[0], dtype=torch.bool)
    keep[sel if sel is not None else torch.arange(R.N)] = False
    assert bool(keep.any())
    assert torch.equal(bits(g.t.cpu()[keep]), bits(init[keep])), f"{name}: a row of dimage outside idx was written"


def image_edge(dtype, op, n, h, w, c, k=0, stride=0, pad=0, mul=1.0, image=None, idx=None, coef=None, a=None, wt1=None, a2=None,
               wt2=None, out=None, dimage=None):
    _check(_lib().mdd_op_image_edge(DT[dtype], op, n, h, w, c, k, stride, pad, mul, P(image), P(idx), P(coef), P(a), P(wt1),
                                    P(a2), P(wt2), P(out), P(dimage), _stream()))


def vit_glue(dtype, op, n, tok, dim, a, a_t=None, b=None, b_t=None, cls=None, cls_t=None, pos=None, pos_t=None, out=None,
             out_t=None, dcls=None, dpos=None):
    _check(_lib().mdd_op_vit_glue(DT[dtype], op, n, tok, dim, P(a), P(a_t), P(b), P(b_t), P(cls), P(cls_t), P(pos), P(pos_t),
                                  P(out), P(out_t), P(dcls), P(dpos), _stream()))


def resid_op(dtype, op, elems, alpha, beta, c3, c3_t=None, sc=None, sc_t=None, xo=None, xo_t=None, ao=None, ao_t=None):
    _check(_lib().mdd_op_resid(DT[dtype], op, elems, alpha, beta, P(c3), P(c3_t), P(sc), P(sc_t), P(xo), P(xo_t), P(ao), P(ao_t),
                               _stream()))


# (idx given, coef given, mul): the engine's call, coef null, idx null (rows 0 .. n - 1 of the nq)
ACCUM_FORMS = [(True, True, R.MUL), (True, False, 1.0), (False, True, R.MUL)]


def _accum_forms(idx_dev, coef_g):
    for with_idx, with_coef, mul in ACCUM_FORMS:
        tag = f"{'idx' if with_idx else 'noidx'},{'coef' if with_coef else 'nocoef'},mul {mul}"
        yield (idx_dev if with_idx else None, R.IDX if with_idx else None, coef_g.t if with_coef else None,
               R.COEF if with_coef else None, mul, tag)


# ------------------------------------------------------------------------------------------------ image edge
@pytest.mark.parametrize("s,cout,dtype", R.stem_cases())
def test_stem_dgrad_image(s, cout, dtype, report):
    """k_stem_dgrad_image<AT, COUT>: the backward call (one source) and the tangent-backward call (two sources), into a
    random dimage through a non-monotone idx / null idx, coef given / null; the padded weight lanes hold garbage."""
    i, st = R.stem_inputs(s, cout, dtype), R.storage(dtype)
    case = ECase(f"stem dgrad s {s} cout {cout} {dtype}", dtype)
    G = {"dy1": inp(R.nhwc(i["dy1"]), st), "dy2": inp(R.nhwc(i["dy2"]), st), "wt1": inp(R.stem_wt(i["w1"]), st),
         "wt2": inp(R.stem_wt(i["w2"]), st), "coef": inp(torch.tensor([R.COEF]))}
    idx = dev(R.IDX, torch.int64)
    for two in (False, True):
        for ix, sel, cf, cv, mul, tag in _accum_forms(idx, G["coef"]):
            name = f"dimage[{'two' if two else 'one'},{tag}]"
            dimage = Guarded((R.NQ, 3, s, s), init=i["dimage0"])
            image_edge(dtype, 2, R.N, s, s, cout, mul=mul, idx=ix, coef=cf, a=G["dy1"].t, wt1=G["wt1"].t,
                       a2=G["dy2"].t if two else None, wt2=G["wt2"].t if two else None, dimage=dimage.t)
            case.cmp("stem_dgrad", name, dimage, R.stem_ref(s, cout, dtype, two, sel, cv, mul), R.image_rows)
            assert_other_rows_untouched(dimage, i["dimage0"], sel, name)
    assert torch.equal(idx.cpu(), R.IDX)
    for k, t in G.items():
        t.check_untouched(k)
    case.finish(report)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("h,w", R.GS_HW)
def test_image_gather_scatter(h, w, dtype, report):
    """k_img_gather (a copy: bit-exact, channels 3 .. 7 written +0) and k_img_scatter (channels 3 .. 7 hold garbage)."""
    i, st = R.gs_inputs(h, w, dtype), R.storage(dtype)
    case = ECase(f"gather/scatter {h}x{w} {dtype}", dtype)
    image, x0bar, coef = inp(i["image"]), inp(i["x0bar"], st), inp(torch.tensor([R.COEF]))
    idx = dev(R.IDX, torch.int64)
    for ix, sel, tag in ((idx, R.IDX, "idx"), (None, None, "noidx")):
        out = Guarded((R.N, h, w, R.CPAD), st)
        image_edge(dtype, 0, R.N, h, w, R.CPAD, image=image.t, idx=ix, out=out.t)
        ref = R.gather_ref(i["image"], sel)
        assert_bits(out, ref.to(st), f"gather[{tag}]")
        if dtype == "bf16":
            case.cmp("gather_round", f"x0[{tag}]", out, ref, lambda t: t[..., :3].reshape(-1, 3 * w))
    for ix, sel, cf, cv, mul, tag in _accum_forms(idx, coef):
        dimage = Guarded((R.NQ, 3, h, w), init=i["dimage0"])
        image_edge(dtype, 1, R.N, h, w, R.CPAD, mul=mul, idx=ix, coef=cf, a=x0bar.t, dimage=dimage.t)
        case.cmp("scatter", f"dimage[{tag}]", dimage, R.scatter_ref(i["dimage0"], i["x0bar"], sel, cv, mul), R.image_rows)
        assert_other_rows_untouched(dimage, i["dimage0"], sel, f"scatter[{tag}]")
    assert torch.equal(idx.cpu(), R.IDX)
    image.check_untouched("image"), x0bar.check_untouched("x0bar"), coef.check_untouched("coef")
    case.finish(report)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("s,p", R.PATCH_SP)
def test_patchify_unpatchify(s, p, dtype, report):
    """k_patchify (a copy: bit-exact) and k_unpatchify_accum."""
    i, st = R.patch_inputs(s, p, dtype), R.storage(dtype)
    case = ECase(f"patches s {s} p {p} {dtype}", dtype)
    image, colsbar, coef = inp(i["image"]), inp(i["colsbar"], st), inp(torch.tensor([R.COEF]))
    idx = dev(R.IDX, torch.int64)
    for ix, sel, tag in ((idx, R.IDX, "idx"), (None, None, "noidx")):
        out = Guarded(tuple(i["colsbar"].shape), st)
        image_edge(dtype, 3, R.N, s, s, 3, k=p, image=image.t, idx=ix, out=out.t)
        ref = R.patchify_ref(i["image"], sel, p)
        assert_bits(out, ref.float().to(st), f"patchify[{tag}]")
        if dtype == "bf16":
            case.cmp("patchify_round", f"cols[{tag}]", out, ref)
    for ix, sel, cf, cv, mul, tag in _accum_forms(idx, coef):
        dimage = Guarded((R.NQ, 3, s, s), init=i["dimage0"])
        image_edge(dtype, 4, R.N, s, s, 3, k=p, mul=mul, idx=ix, coef=cf, a=colsbar.t, dimage=dimage.t)
        case.cmp("unpatchify", f"dimage[{tag}]", dimage, R.unpatchify_ref(i["dimage0"], i["colsbar"], sel, cv, mul, s, p),
                 R.image_rows)
        assert_other_rows_untouched(dimage, i["dimage0"], sel, f"unpatchify[{tag}]")
    assert torch.equal(idx.cpu(), R.IDX)
    image.check_untouched("image"), colsbar.check_untouched("colsbar"), coef.check_untouched("coef")
    case.finish(report)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("case_", R.IM2COL)
def test_im2col(case_, dtype):
    """k_im2col (a copy: bit-exact; the taps outside the image +0)."""
    h, w, k, stride, pad, cpad = case_
    st = R.storage(dtype)
    x = R.im2col_input(case_, dtype)
    ho, wo = R.im2col_out(h, w, k, stride, pad)
    xin, out = inp(x, st), Guarded((R.IM2COL_N * ho * wo, k * k * cpad), st)
    image_edge(dtype, 5, R.IM2COL_N, h, w, cpad, k=k, stride=stride, pad=pad, a=xin.t, out=out.t)
    ref = R.im2col_ref(x, k, stride, pad)
    assert float((ref == 0).double().mean()) > 0.05          # there are taps outside the image
    assert_bits(out, ref.float().to(st), "col")
    xin.check_untouched("in")


# ------------------------------------------------------------------------------------------------ linear packing
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("launch", list(R.LP_LAUNCHES))
def test_lin_pack(launch, dtype, report):
    """k_lin_pack_all<AT>: the primal call writes every element of wf and wt; the tangent call (theta_t given) writes every
    element of wf_t and wt_t AND of wf and wt again -- all four are compared, all bit-exact (a cast and a transpose).  The
    biases inside theta hold NaN: never read."""
    shapes, st = R.LP_LAUNCHES[launch], R.storage(dtype)
    case = ECase(f"lin_pack {launch} {dtype}", dtype)
    npk = R.lp_descs(shapes)[3]
    theta, theta_t = inp(R.lp_theta(launch)), inp(R.lp_theta(launch, True))
    sh = (C.c_int32 * (2 * len(shapes)))(*[v for s in shapes for v in s])
    ref, ref_t = R.lp_refs(launch), R.lp_refs(launch, True)

    def run(tangent):
        bufs = [Guarded((npk,), st) for _ in range(4 if tangent else 2)]
        _check(_lib().mdd_op_lin_pack(DT[dtype], len(shapes), sh, P(theta.t), P(theta_t.t) if tangent else None, P(bufs[0].t),
                                      P(bufs[1].t), P(bufs[2].t) if tangent else None, P(bufs[3].t) if tangent else None,
                                      _stream()))
        tag = ",tangent call" if tangent else ""
        for g, r, which, name in zip(bufs, ref + ref_t, ("wf", "wt", "wf", "wt"), ("wf", "wt", "wf_t", "wt_t")):
            assert_bits(g, r.float().to(st), name + tag)
            if dtype == "bf16":
                got = g.t.cpu()
                for li, (a, b) in enumerate(zip(R.lp_rows(got, shapes, which), R.lp_rows(r, shapes, which))):
                    case.add("lp_round", f"{name}[{li}]{tag}", R.row_err(a, b))

    run(False), run(True)
    theta.check_untouched("theta"), theta_t.check_untouched("theta_t")
    if dtype == "bf16":
        case.finish(report)


# ------------------------------------------------------------------------------------------------ ViT token glue
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("n,tok,dim", R.GLUE)
def test_vit_glue(n, tok, dim, dtype, report):
    """k_vit_embed, k_vit_embed_bwd, k_add2 (float and Dual), k_cls_gather, k_cls_scatter, k_act_to_f32, k_f32_to_act."""
    i, st = R.glue_inputs(n, tok, dim, dtype), R.storage(dtype)
    case = ECase(f"vit glue n {n} tok {tok} dim {dim} {dtype}", dtype)
    typed = ("pe", "pe_t", "xb", "xb_t", "a", "a_t", "b", "b_t", "c")
    G = {k: inp(v, st if k in typed else torch.float32) for k, v in i.items()}
    T = lambda k: G[k].t
    tokens = lambda t: t.reshape(-1, dim)
    act = lambda *shape: Guarded(shape, st)
    # embed
    x0, x0_t = act(n, tok, dim), act(n, tok, dim)
    vit_glue(dtype, 0, n, tok, dim, T("pe"), cls=T("cls"), pos=T("pos"), out=x0.t)
    case.cmp("embed", "x0", x0, R.embed(i["pe"], i["cls"], i["pos"]), tokens)
    keep = Guarded((n, tok, dim), st, init=x0.t)
    vit_glue(dtype, 0, n, tok, dim, T("pe"), T("pe_t"), cls=T("cls"), cls_t=T("cls_t"), pos=T("pos"), pos_t=T("pos_t"),
             out=keep.t, out_t=x0_t.t)
    case.cmp("embed_t", "x0_t", x0_t, R.embed_tangent(i["pe"], i["pe_t"], i["cls"], i["cls_t"], i["pos"], i["pos_t"]), tokens)
    keep.check_untouched("x0 in the tangent call")
    # embed_bwd: dpos / dcls start as NaN -- they are overwritten, not accumulated into
    peb, peb_t = act(n, tok - 1, dim), act(n, tok - 1, dim)
    dpos, dcls, dpos_t, dcls_t = Guarded((tok, dim)), Guarded((1, dim)), Guarded((tok, dim)), Guarded((1, dim))
    vit_glue(dtype, 1, n, tok, dim, T("xb"), out=peb.t, dcls=dcls.t, dpos=dpos.t)
    ref = R.embed_bwd(i["xb"])
    assert_bits(peb, i["xb"][:, 1:].to(st), "pebar")
    case.cmp("dpos", "dpos", dpos, ref[1]), case.cmp("dcls", "dcls", dcls, ref[2])
    keep = Guarded((n, tok - 1, dim), st, init=peb.t)
    vit_glue(dtype, 1, n, tok, dim, T("xb"), T("xb_t"), out=keep.t, out_t=peb_t.t, dcls=dcls_t.t, dpos=dpos_t.t)
    ref = R.embed_bwd(i["xb_t"])
    assert_bits(peb_t, i["xb_t"][:, 1:].to(st), "pebar_t")
    case.cmp("dpos_t", "dpos_t", dpos_t, ref[1]), case.cmp("dcls_t", "dcls_t", dcls_t, ref[2])
    keep.check_untouched("pebar in the tangent call")
    # class-token rows
    cg, cs = act(n, dim), act(n, tok, dim)
    vit_glue(dtype, 2, n, tok, dim, T("a"), out=cg.t)
    assert_bits(cg, R.cls_gather(i["a"]).to(st), "cls_gather")
    vit_glue(dtype, 3, n, tok, dim, T("c"), out=cs.t)
    assert_bits(cs, R.cls_scatter(i["c"], tok).to(st), "cls_scatter")
    # add2
    o, o_t = act(n, tok, dim), act(n, tok, dim)
    vit_glue(dtype, 4, n, tok, dim, T("a"), b=T("b"), out=o.t)
    case.cmp("add2", "o", o, i["a"].double() + i["b"].double(), tokens)
    keep = Guarded((n, tok, dim), st, init=o.t)
    vit_glue(dtype, 4, n, tok, dim, T("a"), T("a_t"), T("b"), T("b_t"), out=keep.t, out_t=o_t.t)
    case.cmp("add2_t", "o_t", o_t, i["a_t"].double() + i["b_t"].double(), tokens)
    keep.check_untouched("o in the tangent call")
    # conversions
    f, t = Guarded((n, tok, dim)), act(n, tok, dim)
    vit_glue(dtype, 5, n, tok, dim, T("a"), out=f.t)
    assert_bits(f, i["a"], "act_to_f32")
    vit_glue(dtype, 6, n, tok, dim, T("f"), out=t.t)
    assert_bits(t, i["f"].to(st), "f32_to_act")
    if dtype == "bf16":
        case.cmp("f32_to_act_round", "t", t, i["f"].double(), tokens)
    for k, g in G.items():
        g.check_untouched(k)
    case.finish(report)


# ------------------------------------------------------------------------------------------------ residual sums
@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("elems", R.RESID_ELEMS)
def test_resid(elems, dtype, act, report):
    """k_resid_relu / k_resid_silu<float | Dual, AT>: x' and a', without a', their tangents with and without a'_t; no
    element is excluded (the inputs keep x' clear of ReLU's kink)."""
    i, st = R.resid_inputs(elems, dtype), R.storage(dtype)
    case = ECase(f"resid {act} elems {elems} {dtype}", dtype)
    op = 0 if act == "relu" else 1
    G = {k: inp(v, st) for k, v in i.items()}
    T = lambda k: G[k].t
    new = lambda: Guarded((elems,), st)
    x_ref, a_ref = R.resid(i["c3"], i["sc"], act)
    xo, ao = new(), new()
    resid_op(dtype, op, elems, R.ALPHA, R.BETA, T("c3"), sc=T("sc"), xo=xo.t, ao=ao.t)
    case.cmp("resid_x", "x", xo, x_ref, R.flat_rows), case.cmp("resid_a", "a", ao, a_ref, R.flat_rows)
    del x_ref, a_ref
    x_keep, a_keep = Guarded((elems,), st, init=xo.t), Guarded((elems,), st, init=ao.t)
    xt_ref, at_ref = R.resid_tangent(i["c3"], i["c3_t"], i["sc"], i["sc_t"], act)
    xo_t, ao_t = new(), new()
    resid_op(dtype, op, elems, R.ALPHA, R.BETA, T("c3"), T("c3_t"), T("sc"), T("sc_t"), x_keep.t, xo_t.t, a_keep.t, ao_t.t)
    case.cmp("resid_x_t", "x_t", xo_t, xt_ref, R.flat_rows), case.cmp("resid_a_t", "a_t", ao_t, at_ref, R.flat_rows)
    if elems < 1 << 20:          # the forms without the activation output (the last block of a net)
        xo2, xo2_t = new(), new()
        resid_op(dtype, op, elems, R.ALPHA, R.BETA, T("c3"), sc=T("sc"), xo=xo2.t)
        assert_bits(xo2, xo.t.cpu(), "x without a")
        resid_op(dtype, op, elems, R.ALPHA, R.BETA, T("c3"), T("c3_t"), T("sc"), T("sc_t"), x_keep.t, xo2_t.t, a_keep.t, None)
        assert_bits(xo2_t, xo_t.t.cpu(), "x_t without a_t")
    x_keep.check_untouched("x in the tangent call"), a_keep.check_untouched("a in the tangent call")
    for k, g in G.items():
        g.check_untouched(k)
    case.finish(report)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("elems", R.RESID_ELEMS)
def test_scale_act(elems, dtype, report):
    """k_scale<AT>: out = alpha * in."""
    i, st = R.resid_inputs(elems, dtype), R.storage(dtype)
    case = ECase(f"scale elems {elems} {dtype}", dtype)
    src, out = inp(i["c3"], st), Guarded((elems,), st)
    resid_op(dtype, 2, elems, R.ALPHA, 0.0, src.t, xo=out.t)
    case.cmp("scale", "out", out, R.ALPHA * i["c3"].double(), R.flat_rows)
    src.check_untouched("in")
    case.finish(report)


# ------------------------------------------------------------------------------------------------ flat kernels
@pytest.mark.parametrize("n", R.FLAT_N)
def test_flat_vector_kernels(n, report):
    """k_dot (into a non-zero accumulator, both signs), k_scale_out (coef given / null), k_sub_inplace, k_lambda_init."""
    lib, i = _lib(), R.flat_inputs(n)
    case = ECase(f"flat n {n}")
    a, b, coef, dist0 = inp(i["a"]), inp(i["b"]), inp(torch.tensor([R.COEF])), inp(i["dist0"], torch.float64)
    elems = lambda t: t.reshape(-1, 1)
    dot = float(i["a"].double() @ i["b"].double())
    for sign in (1.0, -1.0):
        acc = Guarded((1,), torch.float64, init=i["acc0"])
        _check(lib.mdd_flat_dot(P(a.t), P(b.t), P(acc.t), sign, n, _stream()))
        torch.cuda.synchronize()
        acc.check_sentinels("dot")
        e = abs(float(acc.t.cpu()[0]) - (float(i["acc0"][0]) + sign * dot)) / abs(dot)
        case.add("dot", f"sign {sign:+.0f}", e if e == e else float("inf"))
    for cf, cv, mul in ((coef, R.COEF, R.MUL), (None, None, 0.3)):
        y = Guarded((n,))
        _check(lib.mdd_flat_scale_out(P(y.t), P(a.t), P(cf.t) if cf is not None else None, mul, n, _stream()))
        case.cmp("scale_out", f"y[coef {cv}]", y, R.factor(cv, mul) * i["a"].double(), elems)
    y = Guarded((n,), init=i["y0"])
    _check(lib.mdd_flat_sub_inplace(P(y.t), P(a.t), n, _stream()))
    case.cmp("sub_inplace", "y", y, i["y0"].double() - i["a"].double(), elems)
    lam = Guarded((n,))
    _check(lib.mdd_flat_lambda_init(P(lam.t), P(a.t), P(b.t), P(dist0.t), n, _stream()))
    case.cmp("lambda_init", "lam", lam, R.lambda_init(i["a"], i["b"], i["dist0"]), elems)
    a.check_untouched("a"), b.check_untouched("b"), coef.check_untouched("coef"), dist0.check_untouched("dist0")
    case.finish(report)


def test_flat_scalar_kernels(report):
    """k_match_finalize, k_d2f (overwrite: out starts as NaN and is not read; accumulate; elements past n untouched),
    k_accum_f2d."""
    lib, i = _lib(), R.flat_inputs(1)
    case = ECase("flat scalars")
    s4, d, one = inp(i["s4"], torch.float64), inp(i["d"], torch.float64), inp(i["out0"][:1].clone())
    out3 = Guarded((3,))
    _check(lib.mdd_flat_match_finalize(P(s4.t), P(out3.t), _stream()))
    case.cmp("match_finalize", "losses", out3, R.match_finalize(i["s4"]), lambda t: t.reshape(-1, 1))
    mul = 0.625
    for n in R.D2F_N:
        for accum in (0, 1):
            init = i["out0"].clone()
            if not accum:
                init[:n] = float("nan")
            out = Guarded((64,), init=init)
            _check(lib.mdd_flat_d2f(P(out.t), P(d.t), mul, accum, n, _stream()))
            torch.cuda.synchronize()
            out.check_sentinels("d2f")
            got = out.t.cpu()
            assert torch.equal(bits(got[n:]), bits(init[n:])), "d2f wrote past n"
            ref = (i["out0"][:n].double() if accum else 0.0) + i["d"][:n] * mul
            case.add("d2f", f"n {n} accum {accum}", R.row_err(got[:n].reshape(-1, 1), ref.reshape(-1, 1)))
    for sign in (1.0, -1.0):
        acc = Guarded((1,), torch.float64, init=i["acc0"])
        _check(lib.mdd_flat_accum_f2d(P(acc.t), P(one.t), sign, _stream()))
        case.cmp("accum_f2d", f"sign {sign:+.0f}", acc, i["acc0"] + sign * i["out0"][:1].double())
    s4.check_untouched("s4"), d.check_untouched("d"), one.check_untouched("in")
    case.finish(report)
