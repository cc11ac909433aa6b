"""The float64 references of tests/small_op_refs.py (what tests/test_gpu_small_ops.py compares the kernels with): they
agree with an independent formulation (torch.autograd.functional on the written-out formula, or the closed form), and
at every shape and with the very inputs the GPU tests use, each plausible kernel mistake moves the result by at least
ten times the bound the GPU test applies -- so a kernel that made it could not pass."""
import pytest
import torch
import torch.nn.functional as F
from torch.autograd.functional import jvp as ajvp, vjp as avjp

import small_op_refs as R
from conftest import rel_err

TOL = 1e-12
# the bounds of tests/test_gpu_small_ops.py (its caps; the guards are tighter)
B_F32, B_LIN, B_BF16 = 3e-6, 1e-5, 5e-3
D = lambda t: t.double()


def close(a, b):
    e = rel_err(a, b)
    assert e < TOL, e


# ------------------------------------------------------------------------------------------------ independent formulations
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_references_match_autograd(act):
    i = {k: D(v) for k, v in R.linear_inputs(6, 10, 7).items()}
    x, W, b, dy = i["x"], i["W"], i["b"], i["dy"]
    alpha = 1.0 if act else 0.75
    f = lambda xx, ww, bb: R._act(alpha * torch.einsum("nk,jk->nj", xx, ww) + bb, act)
    y = f(x, W, b)
    close(R.linear_fwd(x, W, b, act, alpha), y)
    close(R.linear_fwd(x, W, None, act, alpha), f(x, W, torch.zeros_like(b)))
    # the tangent contract (act' from the stashed y) IS the derivative of the layer
    _, yt = ajvp(f, (x, W, b), (i["x_t"], i["W_t"], i["b_t"]))
    close(R.linear_fwd_tangent(y, x, i["x_t"], W, i["W_t"], i["b_t"], act, alpha), yt)
    _, yt = ajvp(f, (x, W, b), (torch.zeros_like(x), i["W_t"], torch.zeros_like(b)))
    close(R.linear_fwd_tangent(y, x, None, W, i["W_t"], None, act, alpha), yt)
    # backward passes: closed forms
    close(R.linear_dgrad(dy, W), torch.einsum("nj,jk->nk", dy, W))
    mask = (i["relu_of"] > 0).double()
    close(R.linear_dgrad(dy, W, i["relu_of"]), torch.einsum("nj,jk->nk", dy, W) * mask)
    close(R.linear_dgrad_tangent(dy, i["dy_t"], W, i["W_t"], i["relu_of"]),
          (torch.einsum("nj,jk->nk", i["dy_t"], W) + torch.einsum("nj,jk->nk", dy, i["W_t"])) * mask)
    close(R.linear_dgrad_tangent(dy, None, W, i["W_t"]), torch.einsum("nj,jk->nk", dy, i["W_t"]))
    dW, db = R.linear_wgrad(dy, x)
    _, (dW2, db2) = avjp(lambda ww, bb: torch.einsum("nk,jk->nj", x, ww) + bb, (W, b), dy)
    close(dW, dW2), close(db, db2)
    dWt, dbt = R.linear_wgrad_tangent(dy, i["dy_t"], x, i["x_t"])
    close(dWt, torch.einsum("nj,nk->jk", i["dy_t"], x) + torch.einsum("nj,nk->jk", dy, i["x_t"]))
    close(dbt, i["dy_t"].sum(0))
    dWt, dbt = R.linear_wgrad_tangent(dy, None, x, i["x_t"])
    close(dWt, torch.einsum("nj,nk->jk", dy, i["x_t"]))
    assert float(dbt.abs().max()) == 0.0


def test_pooled_references_match_autograd():
    n, hw, c, ga, beta = 2, 5, 8, 1.7, 0.9
    i = {k: D(v) for k, v in R.pool_inputs("f32", n, hw, c).items()}
    a, a_t, b, b_t, g, g_t, yb, yb_t = (i[k] for k in ("a", "a_t", "b", "b_t", "gate", "gate_t", "ybar", "ybar_t"))
    sig = torch.sigmoid
    close(R.pool_mean(a), a.sum(1) / hw)
    for relu in (False, True):
        act = (lambda t: t.clamp_min(0)) if relu else (lambda t: t * sig(t))
        dact = (lambda t: (t > 0).double()) if relu else (lambda t: sig(t) * (1 + t * (1 - sig(t))))
        pool = lambda t: act(t).sum(1) / hw
        bwd = lambda t, y: y[:, None, :] / hw * dact(t)
        close(R.final_pool(a, relu), pool(a))
        close(R.final_pool_tangent(a, a_t, relu), ajvp(pool, a, a_t)[1])
        close(R.final_pool_bwd(a, yb, relu), bwd(a, yb))
        close(R.final_pool_bwd(a, yb, relu), avjp(pool, a, yb)[1])
        close(R.final_pool_bwd_tangent(a, a_t, yb, yb_t, relu), ajvp(bwd, (a, yb), (a_t, yb_t))[1])
    # squeeze-excite apply: x' = c3 gate ga + sc ; a' = beta silu(x')
    xo = lambda c3, gt, sc: c3 * gt[:, None, :] * ga + sc
    ao = lambda c3, gt, sc: beta * xo(c3, gt, sc) * sig(xo(c3, gt, sc))
    x_ref, a_ref = R.se_apply(a, g, b, ga, beta)
    close(x_ref, xo(a, g, b)), close(a_ref, ao(a, g, b))
    xt_ref, at_ref = R.se_apply_tangent(a, a_t, g, g_t, b, b_t, ga, beta)
    close(xt_ref, ajvp(xo, (a, g, b), (a_t, g_t, b_t))[1]), close(at_ref, ajvp(ao, (a, g, b), (a_t, g_t, b_t))[1])
    # gate gradient: the closed forms of the issue
    zb = lambda xb, c3, gt: (ga * (xb * c3).sum(1)) * gt * (1 - gt)
    cb = lambda xb, c3, gt: xb * gt[:, None, :] * ga
    z_ref, c_ref = R.se_gate_grad(a, b, g, ga)
    close(z_ref, zb(a, b, g)), close(c_ref, cb(a, b, g))
    zt_ref, ct_ref = R.se_gate_grad_tangent(a, a_t, b, b_t, g, g_t, ga)
    close(zt_ref, ajvp(zb, (a, b, g), (a_t, b_t, g_t))[1]), close(ct_ref, ajvp(cb, (a, b, g), (a_t, b_t, g_t))[1])


def _avgpool_loops(x):
    n, h, w, c = x.shape
    out = torch.zeros(n, (h + 1) // 2, (w + 1) // 2, c, dtype=torch.float64)
    for oy in range(out.shape[1]):
        for ox in range(out.shape[2]):
            win = x[:, 2 * oy:min(2 * oy + 2, h), 2 * ox:min(2 * ox + 2, w), :]
            out[:, oy, ox, :] = win.sum((1, 2)) / (win.shape[1] * win.shape[2])
    return out


def test_avgpool_reference_matches_the_window_loops():
    i = R.avgpool_inputs("f32", 2, 5, 3, 4)
    x, dout = D(i["x"]), D(i["dout"])
    close(R.avgpool2(x), _avgpool_loops(x))
    close(R.avgpool2_bwd(dout, 5, 3), avjp(_avgpool_loops, x, dout)[1])


def test_linear_shapes_reach_the_paths_claimed_beside_them():
    plan = lambda form, s: R.lin_mfma_plan(*R.linear_gemm_views(*s)[form])
    S = R.LINEAR_SHAPES
    assert plan("forward", S[0]) == (1, 48) and S[0][1] % 4 == 0 and S[0][1] % 16 != 0
    assert plan("forward", S[1]) == (2, 80) and S[1][1] % 4 != 0 and 80 < S[1][1] < 160
    assert plan("forward", S[2]) == (4, 80) and 240 < S[2][1] < 320 and S[2][0] % 16 == 5 and S[2][0] > 32
    assert plan("forward", S[3]) == (8, 80) and 6 * 80 < S[3][1] <= 7 * 80          # wave 7 starts past K
    assert plan("forward", S[4]) == (8, 192)
    assert plan("forward", S[5]) == (1, 384)
    assert plan("dgrad", S[4]) == (4, 96) and plan("dgrad", S[5]) == (4, 384)
    assert plan("wgrad", S[5])[0] == 1 and plan("wgrad", S[6]) == (4, 128)
    reached = {form: {plan(form, s)[0] for s in S} for form in ("forward", "dgrad", "wgrad")}
    assert reached == {"forward": {1, 2, 4, 8}, "dgrad": {1, 4}, "wgrad": {1, 4}}
    assert {b for b, _, _ in S} >= {5, 10, 37, 100, 500}                             # K of the weight-gradient form
    for s in R.MISALIGNED_SHAPES:
        assert s in S and s[1] % 4 == 0
    assert {plan("forward", s)[0] for s in R.MISALIGNED_SHAPES} == {1, 4}
    # the tiled broadcast kernels: c a multiple of 32 sixteen-byte chunks, rows per block = ceil(hw / splits) up to 8
    rows = lambda hw: (((hw + (hw + 63) // 64 - 1) // ((hw + 63) // 64)) + 7) & ~7
    assert (rows(196), -(-196 // rows(196))) == (56, 4) and rows(49) == 56 and (rows(65), -(-65 // rows(65))) == (40, 2)
    for dtype, ce in (("f32", 4), ("bf16", 8)):
        assert [c for c in R.POOL_C if c % ce == 0 and (c // ce) % 32 == 0][0] == R.TILED_C[dtype]
    cases = R.pool_cases()
    for dtype in ("f32", "bf16"):
        have = {(hw, c) for d, _, hw, c in cases if d == dtype}
        assert all((hw, 40) in have and (hw, R.TILED_C[dtype]) in have for hw in R.POOL_HW)
        assert all((hw, c) in have for hw in (1, 49) for c in R.POOL_C)
    assert {n for _, n, _, _ in cases} == {1, 3}


# ------------------------------------------------------------------------------------------------ wrong variants
def far(wrong, ref, bound):
    e = rel_err(wrong, ref)
    assert e >= 10 * bound, (e, bound)


@pytest.mark.parametrize("batch,k,j", R.LINEAR_SHAPES + R.ROUTE1_SHAPES)
def test_linear_inputs_expose_wrong_kernels(batch, k, j):
    i = R.linear_inputs(batch, k, j)
    x, x_t, W, W_t, b, b_t, dy, dy_t, ro = (i[n] for n in ("x", "x_t", "W", "W_t", "b", "b_t", "dy", "dy_t", "relu_of"))
    # last k index dropped, in each form's contraction
    for act in (0, 1, 2):
        far(R.linear_fwd(x[:, :-1], W[:, :-1], b, act), R.linear_fwd(x, W, b, act), B_LIN)
        y = R.linear_fwd(x, W, b, act)
        far(R.linear_fwd_tangent(y, x[:, :-1], x_t[:, :-1], W[:, :-1], W_t[:, :-1], b_t, act),
            R.linear_fwd_tangent(y, x, x_t, W, W_t, b_t, act), B_LIN)
        # A B_t omitted
        far(R.linear_fwd_tangent(y, x, x_t, W, None, b_t, act), R.linear_fwd_tangent(y, x, x_t, W, W_t, b_t, act), B_LIN)
    if (batch, k, j) in R.ROUTE1_SHAPES:
        return
    for mask in (None, ro):
        far(R.linear_dgrad(dy[:, :-1], W[:-1], mask), R.linear_dgrad(dy, W, mask), B_LIN)
        far(R.linear_dgrad_tangent(dy[:, :-1], dy_t[:, :-1], W[:-1], W_t[:-1], mask),
            R.linear_dgrad_tangent(dy, dy_t, W, W_t, mask), B_LIN)
        far(R.linear_dgrad_tangent(dy, dy_t, W, None, mask), R.linear_dgrad_tangent(dy, dy_t, W, W_t, mask), B_LIN)
    dW, db = R.linear_wgrad(dy, x)
    dWt, dbt = R.linear_wgrad_tangent(dy, dy_t, x, x_t)
    # last k (= batch row) dropped: the weight gradient, and the bias-gradient sum missing its last row
    far(R.linear_wgrad(dy[:-1], x[:-1])[0], dW, B_LIN)
    far(R.linear_wgrad(dy[:-1], x[:-1])[1], db, B_LIN)
    w_t, wb_t = R.linear_wgrad_tangent(dy[:-1], dy_t[:-1], x[:-1], x_t[:-1])
    far(w_t, dWt, B_LIN), far(wb_t, dbt, B_LIN)
    far(R.linear_wgrad_tangent(dy, dy_t, x, None)[0], dWt, B_LIN)
    # the accumulating form adds to non-zero dW / db: the same mistakes, seen behind what was there
    far(i["dW0"].double() + R.linear_wgrad(dy[:-1], x[:-1])[0], i["dW0"].double() + dW, B_LIN)
    far(i["db0"].double() + R.linear_wgrad(dy[:-1], x[:-1])[1], i["db0"].double() + db, B_LIN)
    far(i["dW0"].double() + R.linear_wgrad_tangent(dy, dy_t, x, None)[0], i["dW0"].double() + dWt, B_LIN)


@pytest.mark.parametrize("dtype,n,hw,c", R.pool_cases())
def test_pooled_inputs_expose_wrong_kernels(dtype, n, hw, c):
    i = R.pool_inputs(dtype, n, hw, c)
    a, a_t, b, b_t, g, g_t = (i[k] for k in ("a", "a_t", "b", "b_t", "gate", "gate_t"))
    ga, beta = 1.7, 0.9
    stored = B_F32 if dtype == "f32" else B_BF16
    cut = lambda t: t[:, :-1]
    sc = (hw - 1) / hw
    # last hw row dropped from each reduction (fp32 outputs)
    far(R.pool_mean(cut(a)) * sc if hw > 1 else torch.zeros(n, c), R.pool_mean(a), B_F32)
    for relu in (False, True):
        far(R.final_pool(cut(a), relu) * sc if hw > 1 else torch.zeros(n, c), R.final_pool(a, relu), B_F32)
        far(R.final_pool_tangent(cut(a), cut(a_t), relu) * sc if hw > 1 else torch.zeros(n, c),
            R.final_pool_tangent(a, a_t, relu), B_F32)
    z, _ = R.se_gate_grad(a, b, g, ga)
    zt, _ = R.se_gate_grad_tangent(a, a_t, b, b_t, g, g_t, ga)
    if hw > 1:
        far(R.se_gate_grad(cut(a), cut(b), g, ga)[0], z, B_F32)
        far(R.se_gate_grad_tangent(cut(a), cut(a_t), cut(b), cut(b_t), g, g_t, ga)[0], zt, B_F32)
    else:
        far(torch.zeros(n, c), z, B_F32), far(torch.zeros(n, c), zt, B_F32)
    # gate (1 - gate) replaced by gate
    far(z / (1 - g.double()), z, B_F32)
    dgate = z / (g.double() * (1 - g.double()))          # ga sum_hw xbar c3
    dgate_t = (zt - dgate * (1 - 2 * g.double()) * g_t.double()) / (g.double() * (1 - g.double()))
    far(dgate_t * g.double() + dgate * g_t.double(), zt, B_F32)
    # the tangent of sc ignored
    xt, at = R.se_apply_tangent(a, a_t, g, g_t, b, b_t, ga, beta)
    xw, aw = R.se_apply_tangent(a, a_t, g, g_t, b, None, ga, beta)
    far(xw, xt, stored), far(aw, at, stored)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n,h,w,c", R.AVGPOOL_SHAPES)
def test_avgpool_inputs_expose_a_window_divided_by_four(n, h, w, c, dtype):
    i = R.avgpool_inputs(dtype, n, h, w, c)
    x, dout = D(i["x"]), D(i["dout"])
    stored = B_F32 if dtype == "f32" else B_BF16
    # every window divided by 4: zero padding to even sizes, then the plain pool and its backward
    xp = F.pad(x, (0, 0, 0, w % 2, 0, h % 2))
    fwd_wrong = R.avgpool2(xp)
    bwd_wrong = R.avgpool2_bwd(dout, xp.shape[1], xp.shape[2])[:, :h, :w]
    if h % 2 == 0 and w % 2 == 0:        # no ragged window at this shape: the two coincide, nothing to expose
        close(fwd_wrong, R.avgpool2(x)), close(bwd_wrong, R.avgpool2_bwd(dout, h, w))
    else:
        far(fwd_wrong, R.avgpool2(x), stored), far(bwd_wrong, R.avgpool2_bwd(dout, h, w), stored)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """mdd_op_linear / mdd_op_pool_se / mdd_op_weight_std / mdd_op_text_head / mdd_op_contrastive validate on the host:
    none of these calls reaches a kernel (no GPU needed)."""
    import ctypes as C
    import os
    from multimodal_dataset_distillation_amd import _lib, build_ext
    if not os.path.exists(_lib.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _lib.load()
    p = C.c_void_p(64)      # never dereferenced: every call below fails its argument check
    lin = lambda form, route, wdt, act, b=None, out_t=None, out=p: lib.mdd_op_linear(
        form, route, wdt, 4, 8, 4, act, 1.0, p, None, p, None, b, None, p, None, None, out, out_t, None, None)
    assert lin(5, 0, 0, 0) == 2 and b"invalid argument" in lib.mdd_last_error()
    assert lin(0, 2, 0, 0) == 2
    assert lin(0, 0, 1, 0) == 2            # bf16 weights belong to form 3
    assert lin(1, 0, 0, 1) == 2            # an activation belongs to form 0
    assert lin(0, 0, 0, 0, out=None) == 2
    assert lin(1, 1, 0, 0) == 2 and lin(0, 1, 0, 1) == 2 and lin(0, 1, 0, 0, b=p) == 2 and lin(0, 1, 0, 0, out_t=p) == 2
    pool = lambda dtype, op, c, a_t=None, out_t=None, v=p: lib.mdd_op_pool_se(
        dtype, op, 1, 2, 2, c, 1.0, 1.0, p, a_t, p, None, v, None, p, out_t, p, None, None)
    assert pool(2, 0, 8) == 2 and pool(0, 9, 8) == 2
    assert pool(0, 0, 6) == 2 and pool(1, 0, 12) == 2          # channels: whole 16-byte chunks
    assert pool(0, 7, 8, a_t=p) == 2                            # the average pool has no tangent form
    assert pool(0, 1, 8, a_t=p) == 2 and pool(0, 1, 8, out_t=p) == 2    # tangent operands come together
    assert pool(0, 3, 8, v=None) == 2
    # weight standardisation: dtype, mode, geometry, which buffers belong to which mode, whole 16-byte chunks
    err = lambda: lib.mdd_last_error()
    convs = lambda *rows: (_lib.MddWsConv * len(rows))(*[_lib.MddWsConv(*r) for r in rows])
    ok = convs((16, 3, 3, 1, 8))
    ws = lambda dtype=0, mode=0, n=1, cv=ok, th=p, th_t=None, wf=p, wt=p, wf_t=None, wt_t=None, dwf=None, dwf_t=None, g=None: \
        lib.mdd_op_weight_std(dtype, mode, n, cv, 1.7, 1e-5, th, th_t, wf, wt, wf_t, wt_t, dwf, dwf_t, g, None)
    assert ws(dtype=2) == 2 and b"invalid argument" in err() and ws(mode=2) == 2 and ws(n=0) == 2 and ws(th=None) == 2
    assert ws(wt=None) == 2 and ws(wf_t=p) == 2 and ws(dwf=p) == 2 and ws(g=p) == 2
    assert ws(th_t=p) == 2 and ws(th_t=p, wf_t=p, wt_t=p, wt=None) == 2       # tangent: wf_t and wt_t; wf / wt both or neither
    assert ws(mode=1) == 2 and ws(mode=1, wf=None, wt=None, dwf=p) == 2 and ws(mode=1, wf=None, wt=None, dwf=p, g=p, dwf_t=p) == 2
    assert ws(mode=1, dwf=p, g=p) == 2                                          # backward takes no packed weights
    assert ws(cv=convs((16, 3, 3, 1, 2))) == 2 and ws(cv=convs((16, 4, 3, 3, 9))) == 2 and ws(cv=convs((0, 3, 3, 1, 8))) == 2
    assert ws(cv=convs((16, 3, 3, 1, 6))) == 2 and b"16-byte chunk" in err()   # cin_pad: whole chunks
    assert ws(dtype=1, cv=convs((12, 8, 3, 1, 8))) == 2 and ws(n=2, cv=convs((16, 3, 3, 1, 8), (16, 8, 1, 1, 9))) == 2
    # text head: op range, tangent operands together, operands that belong to other ops
    th = lambda op, a=p, a_t=None, b=None, b_t=None, c=None, c_t=None, mask=None, gamma=None, gamma_t=None, beta=None, \
        beta_t=None, idx=None, coef=None, out=p, out_t=None, out2=None, out2_t=None, dg=None, db=None, stats=None, n=2, d=8: \
        lib.mdd_op_text_head(op, n, d, 1e-5, 1.0, a, a_t, b, b_t, c, c_t, mask, gamma, gamma_t, beta, beta_t, idx, coef, out,
                             out_t, out2, out2_t, dg, db, stats, None)
    assert th(6) == 2 and b"invalid argument" in err() and th(-1) == 2 and th(0, n=0) == 2 and th(0, a=None) == 2
    assert th(0, out_t=p) == 2 and th(0, a_t=p) == 2 and th(0, b=p) == 2 and th(0, gamma=p) == 2 and th(0, idx=p) == 2
    assert th(1) == 2 and th(1, b=p, c=p, a_t=p, out_t=p) == 2 and th(1, b=p, c=p, b_t=p) == 2
    assert th(2, b=p, gamma=p, beta=p) == 2 and th(2, b=p, gamma=p, beta=p, out2=p, dg=p) == 2
    assert th(2, b=p, gamma=p, beta=p, out2=p, a_t=p, out_t=p, b_t=p) == 2      # the tangent needs r_t
    assert th(2, b=p, gamma=p, beta=p, out2=p, gamma_t=p) == 2                  # a tangent operand in a primal call
    assert th(3, b=p, gamma=p, out2=p, dg=p, db=p) == 2 and th(3, b=p, gamma=p, out2=p, dg=p, db=p, stats=p, beta=p) == 2
    assert th(4, a_t=p, out_t=p) == 2 and th(4, coef=p) == 2 and th(5, b=p) == 2 and th(4, mask=p) == 2
    # contrastive head: what its kernels cannot take (d > 4096, the LDS request of n, n * n past int)
    con = lambda n, d: lib.mdd_op_contrastive(n, d, p, p, None, None, None, 0.7, p, p, p, p, p, None)
    assert con(4, 4097) == 2 and b"d > 4096" in err()
    assert con(4093, 8) == 2 and b"64 KiB" in err()
    assert con(46341, 8) == 2 and b"overflows int" in err()
    assert con(0, 8) == 2 and con(4, 0) == 2
