"""The float64 references of tests/head_ws_refs.py (what tests/test_gpu_head_ws.py compares the kernels with): they agree
with an independent formulation (torch.autograd.functional on the written-out closed forms, oracle.nfnet_ref's
standardised convolution, oracle.distill_ref's loss), the shapes reach what is claimed beside them, and with the very
inputs the GPU tests use each plausible kernel mistake moves the affected output by at least ten times the cap the GPU
test applies to it -- so a kernel that made it could not pass."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch.autograd.functional import jvp as ajvp, vjp as avjp

import head_ws_refs as R
from conftest import rel_err

TOL = 1e-12
# the caps of tests/test_gpu_head_ws.py (its guards are tighter)
B_F32, B_BF16, B_CON = 3e-6, 5e-3, 1e-4
D = lambda t: t.double()


def close(a, b):
    e = rel_err(a, b)
    assert e < TOL, e


def far(wrong, ref, bound, err=R.row_err):
    e = err(wrong, ref)
    assert e >= 10 * bound, (e, bound)


# ------------------------------------------------------------------------------------------------ weight standardisation
def _ws_variant(w, gain, variant, cin_pad_fan=None, gamma=R.WS_GAMMA, eps=R.WS_EPS):
    """the written-out formula, with the mistakes a kernel could make"""
    cout, fan = w.shape[0], w[0].numel()
    r = w.reshape(cout, fan)
    nmean = cin_pad_fan if variant == "mean_over_cin_pad" else fan
    mu = r.sum(1, keepdim=True) / nmean
    q = ((r - mu) ** 2).sum(1, keepdim=True)
    var = q / (fan - 1 if variant == "unbiased" else nmean)
    rstd = 1 / (var.sqrt() + eps) if variant == "eps_outside" else (var + eps) ** -0.5
    return ((r - mu) * rstd * gain[:, None] * gamma * fan ** -0.5).reshape(w.shape)


def _ws_bwd_closed(w, gain, dwh, gamma=R.WS_GAMMA, eps=R.WS_EPS):
    """csrc/ws.hip: u = (w - mu) rstd, dgain = scale sum(dwh u), dw = gain scale rstd (dwh - mean(dwh) - u mean(dwh u))"""
    cout, fan = w.shape[0], w[0].numel()
    r, g = w.reshape(cout, fan), dwh.reshape(cout, fan)
    mu = r.mean(1, keepdim=True)
    rstd = (((r - mu) ** 2).mean(1, keepdim=True) + eps) ** -0.5
    u = (r - mu) * rstd
    scale = gamma / math.sqrt(fan)
    dgain = scale * (g * u).sum(1)
    dw = gain[:, None] * scale * rstd * (g - g.mean(1, keepdim=True) - u * (g * u).mean(1, keepdim=True))
    return dw.reshape(w.shape), dgain


def _all_ws_outputs(i, f):
    """(wh, wh_t, dw, dgain, dw_t, dgain_t) of a standardisation f(w, gain), through torch.autograd.functional"""
    w, w_t, gain, gain_t, dwh, dwh_t = (D(i[k]) for k in ("w", "w_t", "gain", "gain_t", "dwh", "dwh_t"))
    bwd = lambda a, b, c: avjp(f, (a, b), c, create_graph=True)[1]
    wh, wh_t = ajvp(f, (w, gain), (w_t, gain_t))
    (dw, dgain), (dw_t, dgain_t) = ajvp(bwd, (w, gain, dwh), (w_t, gain_t, dwh_t))
    return dict(wh=wh, wh_t=wh_t, dw=dw, dgain=dgain, dw_t=dw_t, dgain_t=dgain_t)


@pytest.mark.parametrize("shape", R.WS_SHAPES)
def test_ws_references_match_autograd_the_closed_forms_and_the_oracle(shape):
    from oracle import nfnet_ref as nr
    cout, cin, k, groups, cin_pad = shape
    i, ref, p = R.ws_conv_inputs(shape), R.ws_conv_refs(shape), R.ws_plan(shape)
    w, w_t, gain, gain_t, dwh, dwh_t = (D(i[n]) for n in ("w", "w_t", "gain", "gain_t", "dwh", "dwh_t"))
    # torch.autograd.functional on the written-out formula
    alt = _all_ws_outputs(i, lambda a, b: _ws_variant(a, b, "right"))
    for name in alt:
        close(ref[name], alt[name])
    # the closed forms of the backward pass, and their directional derivative
    dw, dgain = _ws_bwd_closed(w, gain, dwh)
    close(ref["dw"], dw), close(ref["dgain"], dgain)
    _, (dw_t, dgain_t) = ajvp(_ws_bwd_closed, (w, gain, dwh), (w_t, gain_t, dwh_t))
    close(ref["dw_t"], dw_t), close(ref["dgain_t"], dgain_t)
    # the oracle's ScaledStdConv2d: its standardised weight, and its convolution rebuilt from either packed layout
    conv = nr.ScaledStdConv2d(cin, cout, k, groups=groups, gamma=R.WS_GAMMA, eps=R.WS_EPS).double()
    with torch.no_grad():
        conv.weight.copy_(w), conv.gain.copy_(gain.view(-1, 1, 1, 1)), conv.bias.zero_()
        close(ref["wh"], conv.standardized_weight())
        x = torch.randn(2, cin, 5, 5, dtype=torch.float64, generator=R._gen(5, *shape))
        y = conv(x)                                                                  # [2, cout, 5, 5]
        cols = F.unfold(x, k, padding=k // 2).reshape(2, groups, p["cin_g"], k * k, 25)   # (ci, tap) per group
        wf = R.pack_wf(ref["wh"], shape, 0.0).reshape(groups, p["cout_g"], k * k, p["cin_pad_g"])[..., :p["cin_g"]]
        wt = R.pack_wt(ref["wh"], shape, 0.0)[:, :p["cin_g"]]
        close(torch.einsum("gotc,ngctl->ngol", wf, cols).reshape(y.shape), y)
        close(torch.einsum("gcto,ngctl->ngol", wt, cols).reshape(y.shape), y)
    # the padded lanes, and nothing else, keep the fill
    assert int(ref["pad_wf"].sum()) == int(ref["pad_wt"].sum()) == cout * k * k * (p["cin_pad_g"] - p["cin_g"])
    assert R.pack_wf(ref["wh"], shape, 0.0).numel() == R.pack_wt(ref["wh"], shape, 0.0).numel() == p["packed"]
    # the two row views hold the same values per output channel
    close(R.wf_rows(ref["wf"], shape).pow(2).sum(1), R.wt_rows(ref["wt"], shape).pow(2).sum(1))


def test_ws_shapes_reach_what_is_claimed_beside_them():
    a, b, c, d, e, f, g = (R.ws_plan(s) for s in R.WS_SHAPES)
    assert (R.WS_TILE_ROWS, R.WS_SLAB, R.WS_STAT_TRIP) == (16, 64, 512)
    assert a["fan"] == 27 < R.WS_SLAB and a["slabs"] == 1 and (a["cin_g"], a["cin_pad_g"]) == (3, 8)
    assert b["fan"] == 144 and b["tile_rows"] == [16, 8] and b["slabs"] == 3 and b["last_slab"] == 16
    assert c["fan"] == 576 == R.WS_STAT_TRIP + 64 and c["stat_trips"] == 2 and c["last_slab"] == 64
    assert d["cin_g"] == d["cout_g"] == 8 and d["tile_rows"] == [8] and d["tiles"] == 6 and d["fan"] == 72
    assert e["ksq"] == 1 and e["tile_rows"] == [16, 16, 8] and e["fan"] == 104 and e["last_slab"] == 40
    assert f["cout_g"] == f["cin_g"] == 64 and f["tiles"] == 8 and f["tile_rows"] == [16] * 4
    assert g["stat_trips"] == 3 and g["fan"] % R.WS_STAT_TRIP != 0 and g["last_slab"] == 8 and g["tile_rows"] == [16, 8]
    for s in R.WS_SHAPES:
        p = R.ws_plan(s)
        assert s[0] % 4 == 0                                   # k_ws_backward: no block has a row past the last
        assert p["cin_pad_g"] % 8 == 0 and p["cout_g"] % 8 == 0   # whole 16-byte chunks in bf16 (and in fp32)
    assert [p["cin_pad_g"] > p["cin_g"] for p in (a, b, c, d, e, f, g)] == [True] + [False] * 6
    # the launches: all seven, (b) alone, reversed; offsets are prefix sums
    assert R.WS_LAUNCHES["all"] == R.WS_SHAPES and R.WS_LAUNCHES["b_alone"] == [R.WS_SHAPES[1]]
    assert R.WS_LAUNCHES["reversed"] == R.WS_SHAPES[::-1]
    offs, nt, npk = R.ws_offsets(R.WS_SHAPES)
    assert offs[0] == (0, 16 * 27, 0) and offs[1] == (16 * 27 + 16, 16 * 27 + 16 + 24 * 144, 16 * 9 * 8)
    assert nt == R.ws_theta(R.WS_SHAPES).numel() and npk == R.ws_dwf(R.WS_SHAPES).numel()
    # eps moves the small-std conv by more than 1 %
    i = R.ws_conv_inputs(R.WS_SMALL_STD)
    assert R.row_err(R.ws_std(i["w"], i["gain"], eps=0.0), R.ws_conv_refs(R.WS_SMALL_STD)["wh"]) > 0.01


@pytest.mark.parametrize("shape", R.WS_SHAPES)
def test_ws_inputs_expose_wrong_kernels(shape):
    cout, cin, k, groups, cin_pad = shape
    i, ref, p = R.ws_conv_inputs(shape), R.ws_conv_refs(shape), R.ws_plan(shape)
    errs = dict(wh=R.row_err, wh_t=R.row_err, dw=R.row_err, dw_t=R.row_err, dgain=R.gain_err, dgain_t=R.gain_err)

    def all_far(variant, names=tuple(errs)):
        wrong = _all_ws_outputs(i, lambda a, b: _ws_variant(a, b, variant, p["cin_pad_g"] * p["ksq"]))
        for n in names:
            far(wrong[n], ref[n], B_F32, errs[n])

    all_far("unbiased")
    if shape == R.WS_SMALL_STD:
        all_far("eps_outside")
    if p["cin_pad_g"] > p["cin_g"]:
        all_far("mean_over_cin_pad")
    # a dropped gain_t / dwf_t term
    zero = lambda t: torch.zeros_like(t)
    far(R.ws_std_tangent(i["w"], i["w_t"], i["gain"], zero(i["gain"])), ref["wh_t"], B_F32)
    dw_t, dgain_t = R.ws_bwd_tangent(i["w"], i["w_t"], i["gain"], zero(i["gain"]), i["dwh"], i["dwh_t"])
    far(dw_t, ref["dw_t"], B_F32)
    dw_t, dgain_t = R.ws_bwd_tangent(i["w"], i["w_t"], i["gain"], i["gain_t"], i["dwh"], zero(i["dwh"]))
    far(dw_t, ref["dw_t"], B_F32), far(dgain_t, ref["dgain_t"], B_F32, R.gain_err)
    # packing mistakes: visible behind the bf16 cap as well
    for bound in (B_F32, B_BF16):
        for key in ("wh", "wh_t"):
            wh = ref[key]
            if k > 1:      # tap and channel swapped in wt: [g][tap][ci][co] written into the [g][ci][tap][co] buffer
                wrong = R.pack_wt(wh, shape, R.WS_PAD_SENTINEL).permute(0, 2, 1, 3).reshape(-1)
                far(R.wt_rows(wrong, shape), R.wt_rows(R.pack_wt(wh, shape, R.WS_PAD_SENTINEL), shape), bound)
            if p["tile_rows"][-1] < R.WS_TILE_ROWS:        # the last row of a ragged tile missing
                cut = wh.clone()
                cut[p["cout_g"] - 1::p["cout_g"]] = 0
                for pack, rows in ((R.pack_wf, R.wf_rows), (R.pack_wt, R.wt_rows)):
                    far(rows(pack(cut, shape, 0.0), shape), rows(pack(wh, shape, 0.0), shape), bound)
            if p["last_slab"] < R.WS_SLAB:                  # the last weights of a ragged slab missing
                cut = wh.clone().reshape(cout, -1)
                cut[:, p["fan"] - p["last_slab"]:] = 0
                cut = cut.reshape(wh.shape)
                for pack, rows in ((R.pack_wf, R.wf_rows), (R.pack_wt, R.wt_rows)):
                    far(rows(pack(cut, shape, 0.0), shape), rows(pack(wh, shape, 0.0), shape), bound)


# ------------------------------------------------------------------------------------------------ text head
def test_head_references_match_autograd_and_the_closed_forms():
    n, d = 3, 257
    i = {k: (D(v) if v.is_floating_point() else v) for k, v in R.head_inputs(n, d).items()}
    p, p_t, rbar, rbar_t, gbar, gbar_t = (i[k] for k in ("p", "p_t", "rbar", "rbar_t", "gbar", "gbar_t"))
    Phi = lambda t: 0.5 * (1 + torch.erf(t / math.sqrt(2)))
    phi = lambda t: torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)
    close(R.gelu(p), F.gelu(p)), close(R.gelu(p), p * Phi(p))
    close(R.gelu_tangent(p, p_t), (Phi(p) + p * phi(p)) * p_t)
    close(R.gelu_bwd(p, rbar, gbar), rbar + gbar * (Phi(p) + p * phi(p)))
    close(R.gelu_bwd_tangent(p, p_t, rbar, rbar_t, gbar, gbar_t),
          rbar_t + gbar_t * (Phi(p) + p * phi(p)) + gbar * phi(p) * (2 - p * p) * p_t)
    f, f_t, q, q_t, mask, gamma, gamma_t, beta, beta_t, ybar, ybar_t = (
        i[k] for k in ("f", "f_t", "q", "q_t", "mask", "gamma", "gamma_t", "beta", "beta_t", "ybar", "ybar_t"))
    for m in (mask, None):
        mm = m if m is not None else torch.ones_like(f)
        fwd = lambda a, b, c, e: F.layer_norm(a * mm + b, (d,), c, e, R.LN_EPS)
        y, r = R.ln_fwd(f, q, gamma, beta, m)
        close(r, f * mm + q), close(y, fwd(f, q, gamma, beta))
        y_t, r_t = R.ln_fwd_tangent(f, f_t, q, q_t, gamma, gamma_t, beta, beta_t, m)
        close(r_t, f_t * mm + q_t), close(y_t, ajvp(fwd, (f, q, gamma, beta), (f_t, q_t, gamma_t, beta_t))[1])
        y_t0, _ = R.ln_fwd_tangent(f, f_t, q, q_t, gamma, None, beta, None, m)
        close(y_t0, ajvp(fwd, (f, q, gamma, beta), (f_t, q_t, 0 * gamma, 0 * beta))[1])
        # backward: torch.autograd.functional, and the closed form of csrc/head.hip
        rbar_, fbar_, dgamma, dbeta = R.ln_bwd(ybar, r, gamma, m)
        ln = lambda a, c, e: F.layer_norm(a, (d,), c, e, R.LN_EPS)
        _, (rb2, dg2, db2) = avjp(ln, (r, gamma, beta), ybar)
        close(rbar_, rb2), close(fbar_, rb2 * mm), close(dgamma, dg2), close(dbeta, db2)
        close(rbar_, _ln_bwd_closed(ybar, r, gamma))
        bwd = lambda a, b, c: _ln_bwd_closed(a, b, c) * mm
        tan = R.ln_bwd_tangent(ybar, ybar_t, r, r_t, gamma, gamma_t, m)
        close(tan[1], ajvp(bwd, (ybar, r, gamma), (ybar_t, r_t, gamma_t))[1])
        full = lambda a, b, c: avjp(ln, (b, c, beta), a, create_graph=True)[1]
        t2 = ajvp(full, (ybar, r, gamma), (ybar_t, r_t, gamma_t))[1]
        close(tan[0], t2[0]), close(tan[2], t2[1]), close(tan[3], t2[2])


def _ln_bwd_closed(ybar, r, gamma, drop_corr=False, eps=R.LN_EPS):
    """csrc/head.hip: gy = ybar gamma, rbar = rstd (gy - mean(gy) - rhat mean(gy rhat))"""
    mu = r.mean(1, keepdim=True)
    rstd = (((r - mu) ** 2).mean(1, keepdim=True) + eps) ** -0.5
    rhat, gy = (r - mu) * rstd, ybar * gamma
    corr = 0 if drop_corr else rhat * (gy * rhat).mean(1, keepdim=True)
    return rstd * (gy - gy.mean(1, keepdim=True) - corr)


@pytest.mark.parametrize("n,d", R.head_cases())
def test_head_inputs_expose_wrong_kernels(n, d):
    i = R.head_inputs(n, d)
    assert float(i["p"].min()) == -6 and float(i["p"].max()) == 6 and (i["p"] == 0).any()
    assert (i["mask"] == 0).any() and (i["mask"] > 1).any()
    assert sorted(i["idx"].tolist()) != i["idx"].tolist() or n == 1
    assert len(set(i["idx"].tolist())) == n
    f, q, mask, gamma, beta, ybar = (D(i[k]) for k in ("f", "q", "mask", "gamma", "beta", "ybar"))
    y, r = R.ln_fwd(f, q, gamma, beta, mask)
    # mask applied to p as well
    y_wrong, r_wrong = R.ln_fwd((f + q), torch.zeros_like(q), gamma, beta, mask)
    far(r_wrong, r, B_F32), far(y_wrong, y, B_F32)
    # the rhat mean(gy rhat) term dropped from the backward pass
    rbar = R.ln_bwd(ybar, r, gamma, mask)[0]
    far(_ln_bwd_closed(ybar, r, gamma, drop_corr=True), rbar, B_F32)
    # the tangent of gamma ignored, a row missing from the column sums
    tan = R.ln_bwd_tangent(ybar, i["ybar_t"], r, (D(i["f_t"]) * mask + D(i["q_t"])), gamma, i["gamma_t"], mask)
    tan0 = R.ln_bwd_tangent(ybar, i["ybar_t"], r, (D(i["f_t"]) * mask + D(i["q_t"])), gamma, None, mask)
    far(tan0[0], tan[0], B_F32)
    dgamma, dbeta = R.ln_bwd(ybar, r, gamma, mask)[2:]
    if n > 1:
        cut = R.ln_bwd(ybar[:-1], r[:-1], gamma, mask[:-1])
        far(cut[2], dgamma, B_F32, R.elem_err), far(cut[3], dbeta, B_F32, R.elem_err)


# ------------------------------------------------------------------------------------------------ contrastive head
def _con_manual(x, y, s, drop_q=False, skip_last=False, frozen_logits=None):
    """csrc/head.hip written out: (loss, xbar, ybar, sbar), with the mistakes a kernel could make.  frozen_logits: the
    logits the probabilities are taken from, held constant (their tangent dropped)"""
    n = x.shape[0]
    rnx, rny = 1 / x.norm(dim=1, keepdim=True), 1 / y.norm(dim=1, keepdim=True)
    xh, yh = x * rnx, y * rny
    G = xh @ yh.t()
    S = s * (G if frozen_logits is None else frozen_logits)
    lr, lc = torch.logsumexp(S, 1, keepdim=True), torch.logsumexp(S, 0, keepdim=True)
    P, Q = torch.exp(S - lr), torch.exp(S - lc)
    eye = torch.eye(n, dtype=x.dtype)
    Sb = (P + (0 if drop_q else Q) - 2 * eye) / (2 * n)
    loss = ((lr.flatten() + lc.flatten() - 2 * torch.diagonal(S)) / (2 * n)).sum()
    sbar, Gb = (Sb * G).sum(), s * Sb
    keep = n - 1 if skip_last else n
    hx, hy = Gb[:, :keep] @ yh[:keep], Gb[:keep].t() @ xh[:keep]
    xbar = rnx * (hx - xh * (xh * hx).sum(1, keepdim=True))
    ybar = rny * (hy - yh * (yh * hy).sum(1, keepdim=True))
    return loss, xbar, ybar, sbar


@pytest.mark.parametrize("n,d", R.CON_SHAPES)
def test_contrastive_references_and_what_their_inputs_expose(n, d):
    from oracle import distill_ref as dr
    i = R.con_inputs(n, d)
    x, y, x_t, y_t = (D(i[k]) for k in ("x", "y", "x_t", "y_t"))
    for scale in R.CON_SCALES_DEV:
        ref = R.con_refs(n, d, scale)
        s = torch.tensor(R.f32(scale), dtype=torch.float64)
        man = _con_manual(x, y, s)
        names = ("loss", "xbar", "ybar", "sbar")
        if n == 1:          # the degenerate case: everything is exactly zero
            assert all(float(ref[k].abs().max()) == 0.0 for k in ref), ref
            assert all(float(m.abs().max()) < 1e-15 for m in man)
            continue
        for k, m in zip(names, man):
            close(ref[k], m)
        tan = ajvp(lambda a, b: _con_manual(a, b, s)[1:], (x, y), (x_t, y_t))[1]
        for k, m in zip(("xbar_t", "ybar_t", "sbar_t"), tan):
            close(ref[k], m)
        # the fp32 torch evaluation of the oracle's loss on the same inputs: how far a faultless fp32 program is
        xf, yf = i["x"].clone().requires_grad_(True), i["y"].clone().requires_grad_(True)
        sf = torch.tensor(scale, dtype=torch.float32, requires_grad=True)
        L = dr.contrastive_loss(xf, yf, sf)
        gx, gy, gs = torch.autograd.grad(L, (xf, yf, sf), create_graph=True)
        tx, ty = torch.autograd.grad((gx * i["x_t"]).sum() + (gy * i["y_t"]).sum(), (xf, yf),
                                     retain_graph=True)                                           # H v, H symmetric
        e = max(R.row_err(gx, ref["xbar"]), R.row_err(gy, ref["ybar"]), R.row_err(tx, ref["xbar_t"]),
                R.row_err(ty, ref["ybar_t"]))
        assert e <= R.TORCH_F32_ERR["hot" if scale > 1 else "unit"], (scale, e)
        a, b = torch.autograd.grad(gs, (xf, yf))
        gs_t = (a * i["x_t"]).sum() + (b * i["y_t"]).sum()
        for got, k in ((L, "loss"), (gs, "sbar"), (gs_t, "sbar_t")):
            assert R.scalar_err(got.detach(), ref[k]) <= R.TORCH_F32_SCALAR_ERR, (scale, k)
        # mistakes: Q dropped from P + Q - 2 I
        wrong = _con_manual(x, y, s, drop_q=True)
        far(wrong[1], ref["xbar"], B_CON), far(wrong[2], ref["ybar"], B_CON)
        far(wrong[3], ref["sbar"], B_CON, R.scalar_err)
        # the last row of the other side skipped (the 4-row unroll of k_featgrad; no n here is a multiple of 4)
        assert n % 4 != 0
        wrong = _con_manual(x, y, s, skip_last=True)
        far(wrong[1], ref["xbar"], B_CON), far(wrong[2], ref["ybar"], B_CON)
        # the tangent of the scale gradient without its sum(Sbar G_t) term
        Gf = lambda a, b: (a / a.norm(dim=1, keepdim=True)) @ (b / b.norm(dim=1, keepdim=True)).t()
        G, G_t = ajvp(Gf, (x, y), (x_t, y_t))
        S = s * G
        Sb = (torch.softmax(S, 1) + torch.softmax(S, 0) - 2 * torch.eye(n, dtype=torch.float64)) / (2 * n)
        far(ref["sbar_t"] - (Sb * G_t).sum(), ref["sbar_t"], B_CON, R.scalar_err)
        # the tangent of the scaled logits dropped where the probabilities are taken (P_t = Q_t = 0): how far it moves the
        # feature tangents grows with |scale| and falls with n (P - 1 / n is small at scale 0.1), so at the two large
        # batches it clears ten times the cap from |scale| = 0.5 on, at the small ones at every scale; at scale 0.1 with
        # n = 67 and 130 it still stands twice above the cap (and hundreds of times above the guards of the GPU test)
        wrong = ajvp(lambda a, b: _con_manual(a, b, s, frozen_logits=G)[1:3], (x, y), (x_t, y_t))[1]
        if n <= 5 or abs(scale) >= 0.5:
            far(wrong[0], ref["xbar_t"], B_CON), far(wrong[1], ref["ybar_t"], B_CON)
        else:
            assert R.row_err(wrong[0], ref["xbar_t"]) >= 2 * B_CON and R.row_err(wrong[1], ref["ybar_t"]) >= 2 * B_CON
