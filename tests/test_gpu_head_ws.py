"""Weight standardisation (csrc/ws.hip: k_ws_forward<float|Dual, float|bf16>, k_ws_backward<float|Dual>), the text head's
pointwise / LayerNorm / row kernels and the contrastive head (csrc/head.hip, every kernel as float and as Dual) at the op
level (mdd_op_weight_std, mdd_op_text_head, mdd_op_contrastive) against the float64 references of tests/head_ws_refs.py,
evaluated on the same fp32 inputs.

The error of a tensor is the MAXIMUM OVER ROWS of the row's norm-relative error (a row is an output channel for weight
standardisation and a sample for the heads): one wrong channel of one conv, or the last row of a ragged tile, is not
averaged away.  Column sums, the gain gradients and the scalars have measures of their own (head_ws_refs.elem_err,
gain_err, scalar_err).  Every output is a slice of a larger allocation with 64 sentinel elements on either side, which
must come back bit-identical, and starts as NaN; every input, and in tangent calls every primal output, must come back
bit-identical.  tests/test_head_ws_refs_cpu.py shows that with these inputs each plausible kernel mistake moves the
affected output by at least ten times the caps below.

All couts are multiples of 4 (k_ws_backward takes four rows per block), so its `row >= total_rows` guard cannot be
reached through the descriptors the engine or mdd_op_weight_std builds from whole 16-byte chunks: it is not tested."""
import ctypes as C

import pytest
import torch

import head_ws_refs as R
from test_gpu_small_ops import PAD, Case, Guarded, P, _lib, _stream, dev

pytestmark = pytest.mark.gpu

# Caps, from the project: fp32 outputs of reductions and broadcasts 3e-6, tensors stored in bf16 5e-3
# (tests/test_gpu_small_ops.py); the contrastive head, which chains __expf / __logf, the f32 parity bar 1e-4
# (tests/test_gpu_ops.py).
CAP_F32, CAP_BF16, CAP_CON = 3e-6, 5e-3, 1e-4
# Guards per quantity: about twice the largest value measured on MI355X over all cases of this file (each test writes
# every figure to the test report, "head-ws ..." lines), never above the cap.  Measured maxima:
#   weight standardisation, fp32 packing   wf / wt 2.7e-7  wf_t / wt_t 2.6e-7                 (worst conv: (d), fan 72)
#                           bf16 packing   wf / wt 2.1e-3  wf_t / wt_t 2.0e-3                 (the one rounding, 2^-9 at most)
#                           backward       dw 2.6e-7  dgain 5.1e-7  dw_t 2.7e-7  dgain_t 4.9e-7
#   text head   gelu 1.7e-7 / tangent 1.1e-7   gelu_bwd 8.6e-8 / 1.2e-7   scatter 4.7e-8   gather exact
#               ln r 4.7e-8 / 4.9e-8   y 1.2e-7 / 2.7e-7   rbar 2.2e-7 / 4.0e-7   fbar 2.9e-7 / 5.3e-7
#               dgamma 5.6e-7 / 4.1e-7   dbeta 3.6e-7 / 3.7e-7
#   contrastive head, |scale| <= 1   xbar / ybar 3.7e-7  their tangents 3.2e-7  loss 1.5e-7  sbar 1.4e-7  sbar_t 6.1e-7
#                     scale 1 / 0.07 xbar / ybar 4.1e-5  their tangents 4.5e-5  loss 1.5e-5  sbar 2.1e-5  sbar_t 7.9e-6
#                     n = 1          1.4e-6 absolute (ybar_t at scale 1 / 0.07; the reference is exactly zero)
# The contrastive head at |scale| <= 1 is as close to float64 as the fp32 torch evaluation of the same formula (5e-7):
# __expf / __logf cost nothing measurable there.  At scale 1 / 0.07 it is four times further than fp32 torch (1.1e-5), at
# the small batches (n = 3: 4.1e-5, n = 5: 3.7e-5, n = 67 and 130: 5e-6 and 3e-6): the diagonal probability is 0.997 there,
# Sbar = (P + Q - 2 I) / 2n cancels to 3e-3 of its terms, and the error of P -- the argument of __expf carries an
# absolute error of half an ulp of the logit, 14 x 6e-8 -- is amplified three hundred times.  Within the cap; not changed.
# n = 1 is not exactly zero.  The size fits this: k_ce takes the row maximum m as the rounded product s * G and then forms
# s * G - m, which contracts to a fused multiply-add and so returns the rounding residual of s * G (up to 2.4e-7 at a
# logit of 6.4) instead of 0; P - 1 is that residual, and times the scale 14.3 and 1 / |y| it is the 1.4e-6 seen.
# At scale 1 / 0.07 the guards of the feature gradients do not go below four times what the fp32 torch evaluation of the
# same formula reaches on the same inputs (head_ws_refs.TORCH_F32_ERR, asserted on the CPU).
_S = lambda f32, bf16: {"f32": f32, "bf16": bf16}
HOT_FLOOR = 4 * R.TORCH_F32_ERR["hot"]
GUARD = {
    "ws_wf": _S(5.4e-7, 4.2e-3), "ws_wt": _S(5.4e-7, 4.2e-3), "ws_wf_t": _S(5.2e-7, 4.1e-3), "ws_wt_t": _S(5.2e-7, 4.1e-3),
    "ws_dw": 5.3e-7, "ws_dgain": 1.1e-6, "ws_dw_t": 5.5e-7, "ws_dgain_t": 1e-6,
    "gelu": 3.4e-7, "gelu_t": 2.1e-7, "gelu_bwd": 1.8e-7, "gelu_bwd_t": 2.4e-7,
    "ln_r": 1e-7, "ln_y": 2.4e-7, "ln_r_t": 1e-7, "ln_y_t": 5.4e-7,
    "ln_rbar": 4.4e-7, "ln_fbar": 5.8e-7, "ln_rbar_t": 8e-7, "ln_fbar_t": 1.1e-6,
    "ln_dgamma": 1.2e-6, "ln_dbeta": 7.2e-7, "ln_dgamma_t": 8.2e-7, "ln_dbeta_t": 7.5e-7,
    "scatter": 1e-7,
    "con_x": 7.5e-7, "con_x_t": 6.5e-7, "con_loss": 3e-7, "con_sbar": 3e-7, "con_sbar_t": 1.3e-6,
    "con_hot_x": 8.1e-5, "con_hot_x_t": 9e-5, "con_hot_loss": 3e-5, "con_hot_sbar": 4.3e-5, "con_hot_sbar_t": 1.6e-5,
    "con_n1": 3e-6,       # absolute
}


def _guard(kind, dtype):
    g = GUARD[kind]
    return g[dtype] if isinstance(g, dict) else g


def _cap(kind, dtype):
    if kind.startswith("con_"):
        return CAP_CON
    return CAP_BF16 if isinstance(GUARD[kind], dict) and dtype == "bf16" else CAP_F32


assert all(_guard(k, d) <= _cap(k, d) for k in GUARD for d in ("f32", "bf16"))
assert GUARD["con_hot_x"] >= HOT_FLOOR and GUARD["con_hot_x_t"] >= HOT_FLOOR and HOT_FLOOR <= CAP_CON


class HCase(Case):
    """Case with the error measure chosen per comparison, and this file's guards and report prefix"""

    def cmp(self, kind, name, got, ref, err=R.row_err):
        torch.cuda.synchronize()
        got.check_sentinels(name)
        assert tuple(got.t.shape) == tuple(ref.shape), (name, got.t.shape, ref.shape)
        self.add(kind, name, err(got.t, ref))

    def add(self, kind, name, e):
        self.errs.append((kind, name, e))

    def finish(self, report):
        worst = {}
        for k, n, v in self.errs:
            if k not in worst or not v <= worst[k][1]:
                worst[k] = (n, v)
        report(f"head-ws {self.title}: " + " ".join(f"{k}:{n}={v:.2e}" for k, (n, v) in worst.items()))
        for k, (n, v) in worst.items():
            assert v < _guard(k, self.dtype), (self.title, k, n, v, _guard(k, self.dtype))


def inp(t, dtype=torch.float32):
    """an input on the device, between sentinels, to be checked untouched"""
    return Guarded(tuple(t.shape), dtype, init=t)


def _check(rc):
    from multimodal_dataset_distillation_amd._lib import check
    check(rc)


# ------------------------------------------------------------------------------------------------ weight standardisation
_LETTER = {s: "abcdefg"[i] for i, s in enumerate(R.WS_SHAPES)}


def weight_std(dtype, mode, shapes, theta, theta_t=None, wf=None, wt=None, wf_t=None, wt_t=None, dwf=None, dwf_t=None,
               gtheta=None):
    from multimodal_dataset_distillation_amd._lib import MddWsConv
    convs = (MddWsConv * len(shapes))(*[MddWsConv(*s) for s in shapes])
    _check(_lib().mdd_op_weight_std({"f32": 0, "bf16": 1}[dtype], mode, len(shapes), convs, R.WS_GAMMA, R.WS_EPS, P(theta),
                                    P(theta_t), P(wf), P(wt), P(wf_t), P(wt_t), P(dwf), P(dwf_t), P(gtheta), _stream()))


def _packed_buffer(shapes, pad_key, st):
    """the padded lanes hold the sentinel, everything the kernel has to write is NaN"""
    pat = torch.cat([torch.where(R.ws_conv_refs(s)[pad_key], R.WS_PAD_SENTINEL, float("nan")).flatten() for s in shapes])
    return Guarded((pat.numel(),), st, init=pat.to(st))


def _cmp_packed(case, kind, name, g, key, shapes):
    """per conv: the padded lanes bit-identical to the sentinel, the rows (output channels) against the reference"""
    torch.cuda.synchronize()
    g.check_sentinels(name)
    got = g.t.cpu()
    pad_key, rows = ("pad_wf", R.wf_rows) if key.startswith("wf") else ("pad_wt", R.wt_rows)
    for s, (_, _, op) in zip(shapes, R.ws_offsets(shapes)[0]):
        ref, pad = R.ws_conv_refs(s)[key], R.ws_conv_refs(s)[pad_key]
        blk = got[op:op + ref.numel()].view(ref.shape)
        lanes = blk[pad]
        assert torch.equal(lanes, torch.full_like(lanes, R.WS_PAD_SENTINEL)), f"{name}[{_LETTER[s]}]: a padded lane was written"
        z = lambda t: torch.where(pad, torch.zeros((), dtype=torch.float64), t.double())
        case.add(kind, f"{name}[{_LETTER[s]}]", R.row_err(rows(z(blk), s), rows(z(ref), s)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("launch", list(R.WS_LAUNCHES))
def test_weight_std_forward(launch, dtype, report):
    """k_ws_forward<float, AT> and <Dual, AT>: both packed layouts of every conv of the launch, the tangent call with and
    without the primal buffers."""
    shapes, st = R.WS_LAUNCHES[launch], R.storage(dtype)
    case = HCase(f"ws forward {launch} {dtype}", dtype)
    theta, theta_t = inp(R.ws_theta(shapes)), inp(R.ws_theta(shapes, "w_t", "gain_t"))
    new = lambda: (_packed_buffer(shapes, "pad_wf", st), _packed_buffer(shapes, "pad_wt", st))
    wf, wt = new()
    weight_std(dtype, 0, shapes, theta.t, wf=wf.t, wt=wt.t)
    _cmp_packed(case, "ws_wf", "wf", wf, "wf", shapes), _cmp_packed(case, "ws_wt", "wt", wt, "wt", shapes)
    for with_primal in (True, False):
        tag = "+primal" if with_primal else ""
        (wf, wt), (wf_t, wt_t) = new(), new()
        weight_std(dtype, 0, shapes, theta.t, theta_t.t, wf=wf.t if with_primal else None, wt=wt.t if with_primal else None,
                   wf_t=wf_t.t, wt_t=wt_t.t)
        _cmp_packed(case, "ws_wf_t", "wf_t" + tag, wf_t, "wf_t", shapes)
        _cmp_packed(case, "ws_wt_t", "wt_t" + tag, wt_t, "wt_t", shapes)
        if with_primal:
            _cmp_packed(case, "ws_wf", "wf" + tag, wf, "wf", shapes), _cmp_packed(case, "ws_wt", "wt" + tag, wt, "wt", shapes)
    theta.check_untouched("theta"), theta_t.check_untouched("theta_t")
    case.finish(report)


def _cmp_gtheta(case, sfx, g, shapes):
    torch.cuda.synchronize()
    g.check_sentinels("gtheta" + sfx)
    got = g.t.cpu()
    assert bool(torch.isfinite(got).all()), "gtheta: an element was not written, or a padded lane of dwf was read"
    for s, (ow, og, _) in zip(shapes, R.ws_offsets(shapes)[0]):
        ref = R.ws_conv_refs(s)
        case.add("ws_dw" + sfx, f"dw{sfx}[{_LETTER[s]}]", R.row_err(got[ow:og].view(ref["dw"].shape), ref["dw" + sfx]))
        case.add("ws_dgain" + sfx, f"dgain{sfx}[{_LETTER[s]}]", R.gain_err(got[og:og + s[0]], ref["dgain" + sfx]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("launch", list(R.WS_LAUNCHES))
def test_weight_std_backward(launch, dtype, report):
    """k_ws_backward<float> and <Dual>: the weight gradient and the gain gradient of every conv, compared separately; the
    padded lanes of dwf hold NaN and must not be read.  (The kernel is fp32 throughout: dtype only sets the 16-byte chunk
    the descriptors are checked against.)"""
    shapes = R.WS_LAUNCHES[launch]
    case = HCase(f"ws backward {launch} {dtype}", dtype)
    theta, theta_t = inp(R.ws_theta(shapes)), inp(R.ws_theta(shapes, "w_t", "gain_t"))
    dwf, dwf_t = inp(R.ws_dwf(shapes)), inp(R.ws_dwf(shapes, "dwh_t"))
    nt = R.ws_offsets(shapes)[1]
    g, g_t = Guarded((nt,)), Guarded((nt,))
    weight_std(dtype, 1, shapes, theta.t, dwf=dwf.t, gtheta=g.t)
    _cmp_gtheta(case, "", g, shapes)
    weight_std(dtype, 1, shapes, theta.t, theta_t.t, dwf=dwf.t, dwf_t=dwf_t.t, gtheta=g_t.t)
    _cmp_gtheta(case, "_t", g_t, shapes)
    for t, n in ((theta, "theta"), (theta_t, "theta_t"), (dwf, "dwf"), (dwf_t, "dwf_t")):
        t.check_untouched(n)
    case.finish(report)


# ------------------------------------------------------------------------------------------------ text head
def text_head(op, n, d, a, a_t=None, b=None, b_t=None, c=None, c_t=None, mask=None, gamma=None, gamma_t=None, beta=None,
              beta_t=None, idx=None, coef=None, out=None, out_t=None, out2=None, out2_t=None, dgamma=None, dbeta=None,
              stats=None, mul=1.0):
    _check(_lib().mdd_op_text_head(op, n, d, R.LN_EPS, mul, P(a), P(a_t), P(b), P(b_t), P(c), P(c_t), P(mask), P(gamma),
                                   P(gamma_t), P(beta), P(beta_t), P(idx), P(coef), P(out), P(out_t), P(out2), P(out2_t),
                                   P(dgamma), P(dbeta), P(stats), _stream()))


@pytest.mark.parametrize("n,d", R.head_cases())
def test_text_head_gelu(n, d, report):
    """k_gelu / k_gelu_bwd, float and Dual, over [-6, 6] with 0 and both ends."""
    i = R.head_inputs(n, d)
    case = HCase(f"gelu n {n} d {d}")
    G = {k: inp(i[k]) for k in ("p", "p_t", "rbar", "rbar_t", "gbar", "gbar_t")}
    g, g_t, pb, pb_t = (Guarded((n, d)) for _ in range(4))
    text_head(0, n, d, G["p"].t, out=g.t)
    case.cmp("gelu", "g", g, R.gelu(i["p"]))
    keep = Guarded((n, d), init=g.t)
    text_head(0, n, d, G["p"].t, G["p_t"].t, out=keep.t, out_t=g_t.t)
    case.cmp("gelu_t", "g_t", g_t, R.gelu_tangent(i["p"], i["p_t"]))
    keep.check_untouched("g in the tangent call")
    text_head(1, n, d, G["p"].t, b=G["rbar"].t, c=G["gbar"].t, out=pb.t)
    case.cmp("gelu_bwd", "pbar", pb, R.gelu_bwd(i["p"], i["rbar"], i["gbar"]))
    keep = Guarded((n, d), init=pb.t)
    text_head(1, n, d, G["p"].t, G["p_t"].t, G["rbar"].t, G["rbar_t"].t, G["gbar"].t, G["gbar_t"].t, out=keep.t, out_t=pb_t.t)
    case.cmp("gelu_bwd_t", "pbar_t", pb_t, R.gelu_bwd_tangent(i["p"], i["p_t"], i["rbar"], i["rbar_t"], i["gbar"], i["gbar_t"]))
    keep.check_untouched("pbar in the tangent call")
    for k, t in G.items():
        t.check_untouched(k)
    case.finish(report)


@pytest.mark.parametrize("n,d", R.head_cases())
def test_text_head_layernorm(n, d, report):
    """k_ln_fwd, k_ln_bwd_rows, k_ln_bwd_cols, float and Dual: r = f mask + p with a mask that contains zeros and without
    one, the tangents with and without gamma_t / beta_t."""
    i = R.head_inputs(n, d)
    case = HCase(f"layernorm n {n} d {d}")
    G = {k: inp(i[k]) for k in ("f", "f_t", "q", "q_t", "mask", "gamma", "gamma_t", "beta", "beta_t", "ybar", "ybar_t")}
    T = lambda k: G[k].t
    mat, vec = (lambda: Guarded((n, d))), (lambda: Guarded((d,)))
    for masked in (True, False):
        m, md, tag = (i["mask"], T("mask"), "mask") if masked else (None, None, "nomask")
        y_ref, r_ref = R.ln_fwd(i["f"], i["q"], i["gamma"], i["beta"], m)
        y, r = mat(), mat()
        text_head(2, n, d, T("f"), b=T("q"), mask=md, gamma=T("gamma"), beta=T("beta"), out=y.t, out2=r.t)
        case.cmp("ln_y", f"y[{tag}]", y, y_ref), case.cmp("ln_r", f"r[{tag}]", r, r_ref)
        # the passes below read the stashed r (here: the reference's, in fp32) and must not write it
        r32 = r_ref.float()
        rt_ref32 = R.ln_fwd_tangent(i["f"], i["f_t"], i["q"], i["q_t"], i["gamma"], None, i["beta"], None, m)[1].float()
        stash, y_keep, r_t_in = inp(r32), Guarded((n, d), init=y.t), inp(rt_ref32)
        for params in (True, False):
            gt, bt = (i["gamma_t"], i["beta_t"]) if params else (None, None)
            ptag = tag + (",params_t" if params else "")
            y_t, r_t = mat(), mat()
            text_head(2, n, d, T("f"), T("f_t"), T("q"), T("q_t"), mask=md, gamma=T("gamma"), gamma_t=T("gamma_t") if params else None,
                      beta=T("beta"), beta_t=T("beta_t") if params else None, out=y_keep.t, out_t=y_t.t, out2=stash.t, out2_t=r_t.t)
            yt_ref, rt_ref = R.ln_fwd_tangent(i["f"], i["f_t"], i["q"], i["q_t"], i["gamma"], gt, i["beta"], bt, m)
            case.cmp("ln_y_t", f"y_t[{ptag}]", y_t, yt_ref), case.cmp("ln_r_t", f"r_t[{ptag}]", r_t, rt_ref)
        # backward, from the stashed r
        rb, fb, dg, db, stats = mat(), mat(), vec(), vec(), Guarded((n, 4))
        text_head(3, n, d, T("ybar"), b=stash.t, mask=md, gamma=T("gamma"), out=rb.t, out2=fb.t, dgamma=dg.t, dbeta=db.t,
                  stats=stats.t)
        ref = R.ln_bwd(i["ybar"], r32, i["gamma"], m)
        case.cmp("ln_rbar", f"rbar[{tag}]", rb, ref[0]), case.cmp("ln_fbar", f"fbar[{tag}]", fb, ref[1])
        case.cmp("ln_dgamma", f"dgamma[{tag}]", dg, ref[2], R.elem_err), case.cmp("ln_dbeta", f"dbeta[{tag}]", db, ref[3], R.elem_err)
        stats.check_sentinels("stats")
        rb_keep, fb_keep = Guarded((n, d), init=rb.t), Guarded((n, d), init=fb.t)
        for params in (True, False):
            ptag = tag + (",gamma_t" if params else "")
            rb_t, fb_t, dg_t, db_t, stats = mat(), mat(), vec(), vec(), Guarded((n, 4))
            text_head(3, n, d, T("ybar"), T("ybar_t"), stash.t, r_t_in.t, mask=md, gamma=T("gamma"),
                      gamma_t=T("gamma_t") if params else None, out=rb_keep.t, out_t=rb_t.t, out2=fb_keep.t, out2_t=fb_t.t,
                      dgamma=dg_t.t, dbeta=db_t.t, stats=stats.t)
            ref = R.ln_bwd_tangent(i["ybar"], i["ybar_t"], r32, rt_ref32, i["gamma"], i["gamma_t"] if params else None, m)
            case.cmp("ln_rbar_t", f"rbar_t[{ptag}]", rb_t, ref[0]), case.cmp("ln_fbar_t", f"fbar_t[{ptag}]", fb_t, ref[1])
            case.cmp("ln_dgamma_t", f"dgamma_t[{ptag}]", dg_t, ref[2], R.elem_err)
            case.cmp("ln_dbeta_t", f"dbeta_t[{ptag}]", db_t, ref[3], R.elem_err)
            stats.check_sentinels("stats")
        for t, name in ((stash, "r"), (y_keep, "y"), (r_t_in, "r_t"), (rb_keep, "rbar"), (fb_keep, "fbar")):
            t.check_untouched(f"{name} in the tangent calls [{tag}]")
    for k, t in G.items():
        t.check_untouched(k)
    case.finish(report)


@pytest.mark.parametrize("n,d", R.head_cases())
def test_text_head_gather_scatter(n, d, report):
    """k_gather_rows (a copy: bit-exact) and k_scatter_rows_axpy into non-zero contents: a permutation into a table with
    spare rows, null idx, coef null / given with mul != 1."""
    i = R.head_inputs(n, d)
    case = HCase(f"gather/scatter n {n} d {d}")
    rows = i["table"].shape[0]
    table, src, coef = inp(i["table"]), inp(i["f"]), inp(i["coef"])
    idx = dev(i["idx"], torch.int64)
    for ix, tag in ((idx, "perm"), (None, "noidx")):
        sel = i["idx"] if ix is not None else torch.arange(n)
        out = Guarded((n, d))
        text_head(4, n, d, table.t, idx=ix, out=out.t)
        torch.cuda.synchronize()
        out.check_sentinels(f"gather[{tag}]")
        assert torch.equal(out.t.cpu(), i["table"][sel]), f"gather[{tag}]"
        for cf, mul in ((None, 1.0), (coef, -1.5), (None, 0.625)):
            acc = Guarded((rows, d), init=i["acc0"])
            text_head(5, n, d, src.t, idx=ix, coef=cf.t if cf is not None else None, out=acc.t, mul=mul)
            ref = i["acc0"].double().clone()
            ref[sel] += (mul * (float(i["coef"][0]) if cf is not None else 1.0)) * i["f"].double()
            case.cmp("scatter", f"acc[{tag},coef {cf is not None},mul {mul}]", acc, ref)
            torch.cuda.synchronize()
            untouched = torch.ones(rows, dtype=torch.bool)
            untouched[sel] = False
            assert torch.equal(acc.t.cpu()[untouched], i["acc0"][untouched]), "scatter wrote a row outside idx"
    assert torch.equal(idx.cpu(), i["idx"])
    table.check_untouched("table"), src.check_untouched("in"), coef.check_untouched("coef")
    case.finish(report)


# ------------------------------------------------------------------------------------------------ contrastive head
def contrastive(n, d, x, y, x_t, y_t, scale_dev, scale_const, work, loss, xbar, ybar, sbar):
    _check(_lib().mdd_op_contrastive(n, d, P(x), P(y), P(x_t), P(y_t), P(scale_dev), scale_const, P(work), P(loss), P(xbar),
                                     P(ybar), P(sbar), _stream()))


@pytest.mark.parametrize("n,d", R.CON_SHAPES)
def test_contrastive_head(n, d, report):
    """k_rownorm, k_logits, k_ce, k_featgrad, float and Dual: loss, xbar, ybar, sbar and their tangents at scales 0.1, 0.7,
    -0.5 and 1 / 0.07 through the device scalar and 0.7 through scale_const; (3, 4096) is the largest legal d, n = 1 the
    degenerate case (everything exactly zero in the reference: absolute values)."""
    i = R.con_inputs(n, d)
    case = HCase(f"contrastive n {n} d {d}")
    G = {k: inp(i[k]) for k in ("x", "y", "x_t", "y_t")}
    nws = _lib().mdd_op_contrastive_workspace_floats(n, d)
    assert nws == 4 * n * d + 4 * n + 4 * n * n + 64
    for scale, through_dev in [(s, True) for s in R.CON_SCALES_DEV] + [(0.7, False)]:
        ref = R.con_refs(n, d, scale)
        sd = inp(torch.tensor([scale], dtype=torch.float32)) if through_dev else None
        sc = 0.0 if through_dev else scale          # scale_const is ignored when the device scalar is given
        tag = f"{scale:.3g}{'' if through_dev else ',const'}"
        hot = "hot_" if scale > 1 else ""
        work = Guarded((nws,))
        loss, sbar, sbar_t, xbar, ybar, xbar_t, ybar_t = [Guarded((1,)) for _ in range(3)] + [Guarded((n, d)) for _ in range(4)]
        contrastive(n, d, G["x"].t, G["y"].t, None, None, sd and sd.t, sc, work.t, loss.t, xbar.t, ybar.t, sbar.t)
        torch.cuda.synchronize()
        work.check_sentinels(f"workspace[{tag}]")
        got = dict(loss=loss, xbar=xbar, ybar=ybar, sbar=sbar)
        work = Guarded((nws,))
        loss_keep = Guarded((1,), init=loss.t)
        contrastive(n, d, G["x"].t, G["y"].t, G["x_t"].t, G["y_t"].t, sd and sd.t, sc, work.t, loss_keep.t, xbar_t.t, ybar_t.t,
                    sbar_t.t)
        torch.cuda.synchronize()
        work.check_sentinels(f"workspace[{tag},tangent]")
        loss_keep.check_untouched("loss in the tangent call")
        got.update(xbar_t=xbar_t, ybar_t=ybar_t, sbar_t=sbar_t)
        if n == 1:
            for k, g in got.items():
                g.check_sentinels(k)
                case.add("con_n1", f"{k}[{tag}]", float(torch.nan_to_num(g.t.double().abs().max(), nan=float("inf"))))
                assert float(ref[k].abs().max()) == 0.0
        else:
            for k in ("xbar", "ybar"):
                case.cmp(f"con_{hot}x", f"{k}[{tag}]", got[k], ref[k])
                case.cmp(f"con_{hot}x_t", f"{k}_t[{tag}]", got[k + "_t"], ref[k + "_t"])
            for k in ("loss", "sbar", "sbar_t"):
                case.cmp(f"con_{hot}{k}", f"{k}[{tag}]", got[k], ref[k].reshape(1), R.scalar_err)
        if sd is not None:
            sd.check_untouched("scale")
    for k, t in G.items():
        t.check_untouched(k)
    case.finish(report)
