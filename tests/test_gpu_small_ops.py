"""The small-batch linear layers (csrc/linear.hip: k_lin_mfma through every launcher, k_sgemm_small on the route retrieval
takes) and the pooled / squeeze-excite kernels (csrc/elementwise.hip: k_hw_reduce modes 0-4, the flat and the tiled
broadcast kernels, the ceil-mode average pool and its backward) at the op level (mdd_op_linear, mdd_op_pool_se) against
the float64 references of tests/small_op_refs.py, evaluated on the same (storage-rounded) inputs.

Every output is a slice of a larger allocation with 64 sentinel elements on either side, which must come back
bit-identical (a store past a ragged tile would change them), and is pre-filled with NaN (the accumulating weight
gradient: with the random values the reference adds), so an element the kernel does not write fails the comparison.
tests/test_small_op_refs_cpu.py shows that with these inputs each plausible kernel mistake (a lost k index, a dropped
tangent term, a bias-gradient sum short of a row, a lost hw row, a ragged pool window divided by 4, gate for
gate (1 - gate), a dropped shortcut tangent) moves the result by at least ten times the caps below."""
import ctypes as C
import math

import pytest
import torch

import small_op_refs as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
PAD = 64
GA, BETA = 1.7, 0.9

# Caps, from the project: fp32 outputs of the reductions and broadcasts 3e-6 (tests/test_gpu_nf_regnet.py
# MID_SE_TOL["f32"]); the linear layers 1e-5 (fp32 accumulation of exact products in another order:
# tests/test_gpu_ops.py test_wide_pointwise_wgrad); tensors stored in bf16 5e-3 (MID_SE_TOL["bf16"]).
CAP_F32, CAP_LIN, CAP_BF16 = 3e-6, 1e-5, 5e-3
# Guards per quantity: about twice the largest value measured on MI355X over all cases of this file (each test writes
# every figure to the test report, "small-ops ..." lines), never above the cap.  Measured maxima:
#   linear (fp32)   fwd 3.5e-7  fwd_t 5.0e-7  dgrad 3.6e-7  dgrad_t 5.0e-7  dW 4.0e-7  dW_t 5.7e-7  db 9.8e-8  db_t 9.9e-8
#                   accumulating dW 5.7e-7 db 1.0e-7   typed W fp32 3.5e-7 / tangent 5.0e-7   typed W bf16 3.5e-7 / 5.0e-7
#                   misaligned operands 2.3e-7   route 1 (k_sgemm_small) 2.9e-7
#   fp32 outputs    pool_mean 1.6e-7  final_pool 1.3e-7  final_pool_t 1.5e-7  zbar 1.4e-7  zbar_t 1.9e-7   (either storage)
#   stored, f32     final_pool_bwd 6.7e-8 / tangent 7.5e-8  se x 4.4e-8 / 4.6e-8  se a 7.3e-8 / 8.4e-8  c3bar 4.8e-8 / 6.6e-8
#                   avgpool 4.1e-8  avgpool_bwd 0
#   stored, bf16    final_pool_bwd 2.0e-3 / 2.0e-3  se x 1.7e-3 / 2.1e-3  se a 1.7e-3 / 2.1e-3  c3bar 1.8e-3 / 1.9e-3
#                   avgpool 2.0e-3  avgpool_bwd 0
# bf16 storage: the one rounding of the stored value (2^-9 per element at most) is all there is.  The average pool's
# backward divides by 1, 2 or 4: exact in both formats, so its guard is one fp32 rounding rather than twice zero.
_S = lambda f32, bf16: {"f32": f32, "bf16": bf16}
GUARD = {
    "lin_fwd": 7e-7, "lin_fwd_t": 1e-6, "lin_dgrad": 7e-7, "lin_dgrad_t": 1e-6, "lin_dW": 8e-7, "lin_dW_t": 1.2e-6,
    "lin_db": 2e-7, "lin_db_t": 2e-7, "lin_acc_dW": 1.2e-6, "lin_acc_db": 2e-7,
    "lin_typed_f32": 7e-7, "lin_typed_f32_t": 1e-6, "lin_typed_bf16": 7e-7, "lin_typed_bf16_t": 1e-6,
    "lin_misaligned": 5e-7, "lin_route1": 6e-7,
    "pool_mean": 3.2e-7, "final_pool": 2.6e-7, "final_pool_t": 3e-7, "zbar": 2.8e-7, "zbar_t": 3.8e-7,
    "final_pool_bwd": _S(1.4e-7, 4e-3), "final_pool_bwd_t": _S(1.5e-7, 4e-3),
    "se_x": _S(9e-8, 3.4e-3), "se_x_t": _S(9.2e-8, 4.2e-3), "se_a": _S(1.5e-7, 3.5e-3), "se_a_t": _S(1.7e-7, 4.2e-3),
    "c3bar": _S(1e-7, 3.6e-3), "c3bar_t": _S(1.4e-7, 3.9e-3),
    "avgpool": _S(8.2e-8, 4e-3), "avgpool_bwd": _S(6e-8, 6e-8),
}

def _guard(kind, dtype):
    g = GUARD[kind]
    return g[dtype] if isinstance(g, dict) else g


def _cap(kind, dtype):
    return CAP_LIN if kind.startswith("lin_") else (CAP_BF16 if isinstance(GUARD[kind], dict) and dtype == "bf16" else CAP_F32)


assert all(_guard(k, d) <= _cap(k, d) for k in GUARD for d in ("f32", "bf16"))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(t, dtype=torch.float32, shift=0):
    """t on the device in dtype; shift > 0 places it that many elements past an aligned allocation"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + shift, device=DEV, dtype=dtype)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    return v


class Guarded:
    """A device tensor between two runs of 64 sentinel elements; NaN inside unless init is given."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        self.numel = math.prod(shape)
        self.buf = torch.full((self.numel + 2 * PAD,), -1234.5, device=DEV, dtype=dtype)
        self.t = self.buf[PAD:PAD + self.numel].view(shape)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)
        self.snap = self.buf.clone()

    def _bits(self, t):
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16)

    def check_sentinels(self, name):
        for sl in (slice(0, PAD), slice(PAD + self.numel, None)):
            assert torch.equal(self._bits(self.buf[sl]), self._bits(self.snap[sl])), f"{name}: sentinel overwritten"

    def check_untouched(self, name):
        assert torch.equal(self._bits(self.buf), self._bits(self.snap)), f"{name}: an input was written"


class Case:
    """Collects the comparisons of one test: sentinels, error against the float64 reference, report line, guards."""

    def __init__(self, title, dtype="f32"):
        self.title, self.dtype, self.errs = title, dtype, []

    def cmp(self, kind, name, got, ref):
        torch.cuda.synchronize()
        got.check_sentinels(name)
        assert tuple(got.t.shape) == tuple(ref.shape), (name, got.t.shape, ref.shape)
        self.errs.append((kind, name, rel_err(got.t, ref)))

    def finish(self, report):
        report(f"small-ops {self.title}: " + " ".join(f"{k}:{n}={v:.2e}" for k, n, v in self.errs))
        for k, n, v in self.errs:
            assert v < _guard(k, self.dtype), (self.title, k, n, v, _guard(k, self.dtype))


def _lib():
    from multimodal_dataset_distillation_amd import _lib
    return _lib.load()


def lin(form, route, wdt, n, k, j, act=0, alpha=1.0, x=None, x_t=None, W=None, W_t=None, b=None, b_t=None, dy=None,
        dy_t=None, relu_of=None, out=None, out_t=None, db=None):
    from multimodal_dataset_distillation_amd._lib import check
    check(_lib().mdd_op_linear(form, route, wdt, n, k, j, act, alpha, P(x), P(x_t), P(W), P(W_t), P(b), P(b_t), P(dy),
                               P(dy_t), P(relu_of), P(out), P(out_t), P(db), _stream()))


def pool_se(dtype, op, n, h, w, c, a, a_t=None, b=None, b_t=None, v=None, v_t=None, out=None, out_t=None, out2=None,
            out2_t=None):
    from multimodal_dataset_distillation_amd._lib import check
    check(_lib().mdd_op_pool_se({"f32": 0, "bf16": 1}[dtype], op, n, h, w, c, GA, BETA, P(a), P(a_t), P(b), P(b_t), P(v),
                                P(v_t), P(out), P(out_t), P(out2), P(out2_t), _stream()))


def _drops(names):
    """the full tangent, then each tangent operand dropped to null in turn"""
    yield "full", set()
    for n in names:
        yield f"no_{n}", {n}


# ------------------------------------------------------------------------------------------------ linear layers
def _forward_family(case, kind, form, wdt, wtype, i, batch, k, j, acts, alpha, shift_x=0, shift_w=0, drops=True):
    """forward (form 0) or typed forward (form 3): primal and tangent, with and without bias, every act"""
    x, x_t = dev(i["x"], shift=shift_x), dev(i["x_t"], shift=shift_x)
    W, W_t = dev(i["W"], wtype, shift_w), dev(i["W_t"], wtype, shift_w)
    b, b_t = dev(i["b"]), dev(i["b_t"])
    for act in acts:
        for bias in (True, False):
            tag = f"act{act}{'+b' if bias else ''}"
            y_ref = R.linear_fwd(i["x"], i["W"], i["b"] if bias else None, act, alpha)
            y = Guarded((batch, j))
            lin(form, 0, wdt, batch, k, j, act, alpha, x=x, W=W, b=b if bias else None, out=y.t)
            case.cmp(kind, f"y[{tag}]", y, y_ref)
            # the tangent call reads the stashed post-activation y (here: the reference's, in fp32) and must not write it
            stash = Guarded((batch, j), init=y_ref.float())
            for dn, drop in _drops(["x_t", "W_t"] + (["b_t"] if bias else [])):
                if not drops and dn != "full":
                    continue
                tx = None if "x_t" in drop else (x_t, i["x_t"])
                tw = None if "W_t" in drop else (W_t, i["W_t"])
                tb = None if ("b_t" in drop or not bias) else (b_t, i["b_t"])
                y_t = Guarded((batch, j))
                lin(form, 0, wdt, batch, k, j, act, alpha, x=x, x_t=tx and tx[0], W=W, W_t=tw and tw[0], b=b if bias else None,
                    b_t=tb and tb[0], out=stash.t, out_t=y_t.t)
                ref = R.linear_fwd_tangent(stash.t.cpu(), i["x"], tx and tx[1], i["W"], tw and tw[1], tb and tb[1], act, alpha)
                case.cmp(kind + "_t" if kind != "lin_misaligned" else kind, f"y_t[{tag},{dn}]", y_t, ref)
            stash.check_untouched(f"stash[{tag}]")


@pytest.mark.parametrize("batch,k,j", R.LINEAR_SHAPES)
def test_linear_forward(batch, k, j, report):
    """launch_linear_fwd on the engine's route: act none / ReLU / sigmoid, with and without bias, primal and tangent, each
    tangent operand null in turn."""
    case = Case(f"linear forward n {batch} in {k} out {j}")
    _forward_family(case, "lin_fwd", 0, 0, torch.float32, R.linear_inputs(batch, k, j), batch, k, j, (0, 1, 2), 1.0)
    case.finish(report)


@pytest.mark.parametrize("wdtype", ["f32", "bf16"])
@pytest.mark.parametrize("batch,k,j", R.LINEAR_SHAPES)
def test_linear_typed_forward(batch, k, j, wdtype, report):
    """launch_linear_fwd_w (the pooled-feature -> conv3 shortcut): W in fp32 or bf16 (the reference uses the rounded
    weights), alpha != 1, primal and tangent."""
    case = Case(f"linear typed forward W {wdtype} n {batch} in {k} out {j}")
    _forward_family(case, f"lin_typed_{wdtype}", 3, {"f32": 0, "bf16": 1}[wdtype], R.storage(wdtype),
                    R.linear_inputs(batch, k, j, wdtype), batch, k, j, (0,), 0.625)
    case.finish(report)


@pytest.mark.parametrize("batch,k,j", R.LINEAR_SHAPES)
def test_linear_dgrad(batch, k, j, report):
    """launch_linear_dgrad (A k-contiguous, B strided in k): with and without the ReLU mask, primal and tangent."""
    i = R.linear_inputs(batch, k, j)
    case = Case(f"linear dgrad n {batch} in {k} out {j}")
    dy, dy_t, W, W_t, ro = (dev(i[n]) for n in ("dy", "dy_t", "W", "W_t", "relu_of"))
    for mask in (False, True):
        tag = "mask" if mask else "plain"
        rof, rod = (i["relu_of"], ro) if mask else (None, None)
        dx = Guarded((batch, k))
        lin(1, 0, 0, batch, k, j, dy=dy, W=W, relu_of=rod, out=dx.t)
        case.cmp("lin_dgrad", f"dx[{tag}]", dx, R.linear_dgrad(i["dy"], i["W"], rof))
        for dn, drop in _drops(["dy_t", "W_t"]):
            dx_t = Guarded((batch, k))
            lin(1, 0, 0, batch, k, j, dy=dy, dy_t=None if "dy_t" in drop else dy_t, W=W, W_t=None if "W_t" in drop else W_t,
                relu_of=rod, out=dx.t, out_t=dx_t.t)
            ref = R.linear_dgrad_tangent(i["dy"], None if "dy_t" in drop else i["dy_t"], i["W"],
                                         None if "W_t" in drop else i["W_t"], rof)
            case.cmp("lin_dgrad_t", f"dx_t[{tag},{dn}]", dx_t, ref)
    case.finish(report)


@pytest.mark.parametrize("batch,k,j", R.LINEAR_SHAPES)
def test_linear_wgrad(batch, k, j, report):
    """launch_linear_wgrad and launch_linear_wgrad_accum (both operands strided in k, K = batch): dW and the
    bias-gradient row sums, primal and tangent; the accumulating form into non-zero dW / db."""
    i = R.linear_inputs(batch, k, j)
    case = Case(f"linear wgrad n {batch} in {k} out {j}")
    dy, dy_t, x, x_t = (dev(i[n]) for n in ("dy", "dy_t", "x", "x_t"))
    dW0, db0 = i["dW0"].double(), i["db0"].double()
    for form, kw, kb in ((2, "lin_dW", "lin_db"), (4, "lin_acc_dW", "lin_acc_db")):
        acc = form == 4
        new = lambda: (Guarded((j, k), init=i["dW0"] if acc else None), Guarded((j,), init=i["db0"] if acc else None))
        add = lambda r: (dW0 + r[0], db0 + r[1]) if acc else r
        dW, db = new()
        lin(form, 0, 0, batch, k, j, dy=dy, x=x, out=dW.t, db=db.t)
        rW, rb = add(R.linear_wgrad(i["dy"], i["x"]))
        case.cmp(kw, "dW", dW, rW), case.cmp(kb, "db", db, rb)
        for dn, drop in list(_drops(["dy_t", "x_t"]))[:3]:
            dW, db = new()
            lin(form, 0, 0, batch, k, j, dy=dy, dy_t=None if "dy_t" in drop else dy_t, x=x,
                x_t=None if "x_t" in drop else x_t, out=dW.t, db=db.t)
            rW, rb = add(R.linear_wgrad_tangent(i["dy"], None if "dy_t" in drop else i["dy_t"], i["x"],
                                                None if "x_t" in drop else i["x_t"]))
            case.cmp(kw if acc else kw + "_t", f"dW_t[{dn}]", dW, rW)
            if "dy_t" in drop and not acc:      # db_t = 0 exactly: nothing to divide by
                torch.cuda.synchronize()
                db.check_sentinels("db_t")
                assert float(db.t.abs().max()) == 0.0
            else:
                case.cmp(kb if acc else kb + "_t", f"db_t[{dn}]", db, rb)
    case.finish(report)


@pytest.mark.parametrize("batch,k,j", R.MISALIGNED_SHAPES)
def test_linear_misaligned_operands(batch, k, j, report):
    """K % 4 == 0, so only the pointer alignment takes the 16-byte (bf16: 8-byte) loads away: x one float off, the fp32 W
    one float off, the bf16 W one element off."""
    assert k % 4 == 0
    case = Case(f"linear misaligned n {batch} in {k} out {j}")
    i = R.linear_inputs(batch, k, j)
    _forward_family(case, "lin_misaligned", 0, 0, torch.float32, i, batch, k, j, (2,), 1.0, shift_x=1, drops=False)
    _forward_family(case, "lin_misaligned", 0, 0, torch.float32, i, batch, k, j, (0,), 1.0, shift_w=1, drops=False)
    _forward_family(case, "lin_misaligned", 3, 1, torch.bfloat16, R.linear_inputs(batch, k, j, "bf16"), batch, k, j, (0,),
                    0.625, shift_w=1, drops=False)
    case.finish(report)


@pytest.mark.parametrize("batch,k,j", R.ROUTE1_SHAPES)
def test_linear_route_of_retrieval(batch, k, j, report):
    """launch_linear_fwd with an empty scratch, as retrieval and the caption decode call it: k_sgemm_small, unsplit."""
    i = R.linear_inputs(batch, k, j)
    case = Case(f"linear route 1 n {batch} in {k} out {j}")
    y = Guarded((batch, j))
    lin(0, 1, 0, batch, k, j, x=dev(i["x"]), W=dev(i["W"]), out=y.t)
    case.cmp("lin_route1", "y", y, R.linear_fwd(i["x"], i["W"]))
    case.finish(report)


# ------------------------------------------------------------------------------------------------ pooled / squeeze-excite
@pytest.mark.parametrize("dtype,n,hw,c", R.pool_cases())
def test_pooled_and_squeeze_excite_kernels(dtype, n, hw, c, report):
    """k_hw_reduce modes 0 (mean), 1 / 4 (final pool SiLU / ReLU), 3 (gate gradient + c3bar), the final-pool backward
    and the SE apply (flat kernels, and the tiled ones when c is a multiple of 32 chunks), primal and tangent."""
    st = R.storage(dtype)
    i = R.pool_inputs(dtype, n, hw, c)
    case = Case(f"pooled {dtype} n {n} hw {hw} c {c}", dtype)
    a, a_t, b, b_t = (dev(i[k], st) for k in ("a", "a_t", "b", "b_t"))
    g, g_t, yb, yb_t = (dev(i[k]) for k in ("gate", "gate_t", "ybar", "ybar_t"))
    act = lambda: Guarded((n, hw, c), st)
    vec = lambda: Guarded((n, c))
    h, w = hw, 1

    o = vec()
    pool_se(dtype, 0, n, h, w, c, a, out=o.t)
    case.cmp("pool_mean", "mean", o, R.pool_mean(i["a"]))
    for relu in (False, True):
        tag = "relu" if relu else "silu"
        o, o_t = vec(), vec()
        pool_se(dtype, 2 if relu else 1, n, h, w, c, a, out=o.t)
        pool_se(dtype, 2 if relu else 1, n, h, w, c, a, a_t, out=o.t, out_t=o_t.t)
        case.cmp("final_pool", f"y[{tag}]", o, R.final_pool(i["a"], relu))
        case.cmp("final_pool_t", f"y_t[{tag}]", o_t, R.final_pool_tangent(i["a"], i["a_t"], relu))
        o, o_t = act(), act()
        pool_se(dtype, 4 if relu else 3, n, h, w, c, a, v=yb, out=o.t)
        pool_se(dtype, 4 if relu else 3, n, h, w, c, a, a_t, v=yb, v_t=yb_t, out=o.t, out_t=o_t.t)
        case.cmp("final_pool_bwd", f"cfbar[{tag}]", o, R.final_pool_bwd(i["a"], i["ybar"], relu))
        case.cmp("final_pool_bwd_t", f"cfbar_t[{tag}]", o_t,
                 R.final_pool_bwd_tangent(i["a"], i["a_t"], i["ybar"], i["ybar_t"], relu))
    # SE apply: a = c3, b = sc
    xo, xo_t, ao, ao_t, xo1 = act(), act(), act(), act(), act()
    pool_se(dtype, 5, n, h, w, c, a, b=b, v=g, out=xo.t, out2=ao.t)
    pool_se(dtype, 5, n, h, w, c, a, b=b, v=g, out=xo1.t)                       # the last block: no activation output
    pool_se(dtype, 5, n, h, w, c, a, a_t, b, b_t, g, g_t, out=xo.t, out_t=xo_t.t, out2=ao.t, out2_t=ao_t.t)
    x_ref, a_ref = R.se_apply(i["a"], i["gate"], i["b"], GA, BETA)
    xt_ref, at_ref = R.se_apply_tangent(i["a"], i["a_t"], i["gate"], i["gate_t"], i["b"], i["b_t"], GA, BETA)
    case.cmp("se_x", "x", xo, x_ref), case.cmp("se_x", "x[no_a]", xo1, x_ref), case.cmp("se_a", "a", ao, a_ref)
    case.cmp("se_x_t", "x_t", xo_t, xt_ref), case.cmp("se_a_t", "a_t", ao_t, at_ref)
    # gate gradient: a = xbar, b = c3
    zb, zb_t, cb, cb_t = vec(), vec(), act(), act()
    pool_se(dtype, 6, n, h, w, c, a, b=b, v=g, out=zb.t, out2=cb.t)
    pool_se(dtype, 6, n, h, w, c, a, a_t, b, b_t, g, g_t, out=zb.t, out_t=zb_t.t, out2=cb.t, out2_t=cb_t.t)
    z_ref, c_ref = R.se_gate_grad(i["a"], i["b"], i["gate"], GA)
    zt_ref, ct_ref = R.se_gate_grad_tangent(i["a"], i["a_t"], i["b"], i["b_t"], i["gate"], i["gate_t"], GA)
    case.cmp("zbar", "zbar", zb, z_ref), case.cmp("c3bar", "c3bar", cb, c_ref)
    case.cmp("zbar_t", "zbar_t", zb_t, zt_ref), case.cmp("c3bar_t", "c3bar_t", cb_t, ct_ref)
    case.finish(report)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n,h,w,c", R.AVGPOOL_SHAPES)
def test_ceil_mode_average_pool(n, h, w, c, dtype, report):
    """k_avgpool2 / k_avgpool2_bwd at stride 2 with h and w independent: the ragged last row, column and corner
    (counts 2, 2 and 1) against avg_pool2d(ceil_mode=True, count_include_pad=False) and its vjp."""
    st = R.storage(dtype)
    i = R.avgpool_inputs(dtype, n, h, w, c)
    case = Case(f"avgpool {dtype} n {n} h {h} w {w} c {c}", dtype)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    y, dx = Guarded((n, ho, wo, c), st), Guarded((n, h, w, c), st)
    pool_se(dtype, 7, n, h, w, c, dev(i["x"], st), out=y.t)
    pool_se(dtype, 8, n, h, w, c, dev(i["dout"], st), out=dx.t)
    case.cmp("avgpool", "y", y, R.avgpool2(i["x"]))
    case.cmp("avgpool_bwd", "dx", dx, R.avgpool2_bwd(i["dout"], h, w))
    case.finish(report)
