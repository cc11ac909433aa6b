"""Float64 references of the small-batch linear layers (csrc/linear.hip) and of the pooled / squeeze-excite kernels
(csrc/elementwise.hip), with the shapes and the inputs that tests/test_gpu_small_ops.py runs them at and
tests/test_small_op_refs_cpu.py checks them at.  Plain torch: tangents through torch.func.jvp, backward passes through
torch.func.vjp.  Every function computes in float64 whatever it is given; the callers round the inputs to the storage
type first, so that a comparison isolates the kernel."""
import torch
import torch.nn.functional as F
from torch.func import jvp, vjp

F64 = torch.float64

# ------------------------------------------------------------------------------------------------ shapes
# (batch, in, out).  The GEMM view of run_lin_mfma is M x N x K on 16 x 16 tiles with
#   nw = 1; while nw < 8 and tiles * nw < 2048 and K // (2 * nw) >= 64: nw *= 2;  kw_len = roundup16(ceil(K / nw))
# forward / typed forward: M = batch, N = out, K = in, both operands k-contiguous
# dgrad:                   M = batch, N = in,  K = out, A k-contiguous, B strided in k
# wgrad / accumulating:    M = out,   N = in,  K = batch, both operands strided in k
LINEAR_SHAPES = [
    # forward: 1 x 2 tiles (rows 5 of 16, columns 8 of the second), NW 1, K = 40 = 4 * 10 (not a multiple of 16: the
    # 16-byte loads stop inside the second step).  dgrad K = 24, wgrad K = 5: NW 1
    (5, 40, 24),
    # forward: K = 130, K % 4 = 2 -> scalar loads on both operands; 130 // 2 = 65 >= 64 -> NW 2, kw_len 80, wave 1 takes
    # k 80..129 with the ragged tail.  dgrad K = 50, wgrad K = 10: NW 1
    (10, 130, 50),
    # forward: 3 x 6 tiles (M = 37: last tile 5 rows), K = 264: 264 // 4 = 66 >= 64, 264 // 8 = 33 -> NW 4, kw_len 80,
    # wave 3 takes k 240..263 (short).  dgrad K = 96 (96 // 2 < 64): NW 1, N = 264 = 16 * 16 + 8.  wgrad K = 37: NW 1, odd K
    (37, 264, 96),
    # forward: 3 x 2 tiles, K = 520: 520 // 8 = 65 -> NW 8, kw_len 80, wave 6 takes 480..519, wave 7 starts at 560 >= K:
    # empty.  dgrad K = 20, wgrad K = 33
    (33, 520, 20),
    # an NFNet-l0 SE fc1.  forward: 7 x 24 = 168 tiles, K = 1536 -> NW 8, 192 k per wave.  dgrad: 7 x 96 = 672 tiles,
    # K = 384 -> NW 4 (672 * 4 >= 2048 stops it), 96 k per wave.  wgrad K = 100: NW 1
    (100, 1536, 384),
    # forward: 32 x 96 = 3072 tiles >= 2048 -> NW 1, one wave walks K = 384.  dgrad: 32 x 24 = 768 tiles, K = 1536 ->
    # NW 4 (768 * 4 >= 2048), 384 k per wave.  wgrad: 96 x 24 = 2304 tiles >= 2048 -> NW 1 with K = 500 strided
    (500, 384, 1536),
    # wgrad: 3 x 5 = 15 tiles, K = 500: 500 // 4 = 125 >= 64, 500 // 8 = 62 -> NW 4, kw_len 128, wave 3 takes 384..499, both
    # operands strided in k (the shape above keeps NW 1 in this form: too many tiles).  forward K = 72, dgrad K = 40: NW 1
    (500, 72, 40),
]


def lin_mfma_plan(M, N, K):
    """(waves per tile, k per wave) as run_lin_mfma chooses them (csrc/linear.hip) -- restated here so that the
    properties claimed beside the shapes are checked (tests/test_small_op_refs_cpu.py), not only written down"""
    tiles = ((M + 15) // 16) * ((N + 15) // 16)
    nw = 1
    while nw < 8 and tiles * nw < 2048 and K // (nw * 2) >= 64:
        nw *= 2
    return nw, ((K + nw - 1) // nw + 15) // 16 * 16


def linear_gemm_views(batch, k, j):
    """form -> (M, N, K)"""
    return {"forward": (batch, j, k), "dgrad": (batch, k, j), "wgrad": (j, k, batch)}


# route 1 (k_sgemm_small, unsplit, 64 x 64 tiles, 16-deep K steps): one ragged tile with K % 4 != 0 (scalar loads, scalar
# stores); 2 x 3 tiles with 16-byte loads and N % 4 != 0; 3 x 4 tiles, K = 100 (16-byte loads, a K tail of 4), N % 4 == 0
# (16-byte stores)
ROUTE1_SHAPES = [(7, 130, 50), (70, 256, 130), (150, 100, 200)]
# alignment alone switches the scalar loads on: K % 4 == 0 in the forward form, NW 1 and NW 4
MISALIGNED_SHAPES = [(5, 40, 24), (37, 264, 96)]

POOL_HW = [1, 31, 33, 49, 64, 65, 196]
POOL_C = [8, 40, 128, 256]
TILED_C = {"f32": 128, "bf16": 256}     # the first width with a multiple of 32 sixteen-byte chunks


def pool_cases():
    """(dtype, n, hw, c): every hw with c = 40 and with the tiled width of the dtype, every c with hw 1 and 49."""
    out = []
    for dtype in ("f32", "bf16"):
        seen = set()
        for hw in POOL_HW:
            for c in (40, TILED_C[dtype]):
                seen.add((hw, c))
        for hw in (1, 49):
            for c in POOL_C:
                seen.add((hw, c))
        for hw, c in sorted(seen):
            out.append((dtype, 1 if hw in (33, 196) else 3, hw, c))
    return out


# (n, h, w, c): odd in both (ragged row, column and corner), odd and different, a single pixel, even (no ragged
# window), odd rows with even columns
AVGPOOL_SHAPES = [(2, 9, 9, 16), (3, 7, 5, 40), (1, 1, 1, 8), (2, 14, 14, 256), (1, 5, 8, 8)]


# ------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1000003 + int(v)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def storage(dtype):
    return torch.float32 if dtype == "f32" else torch.bfloat16


def linear_inputs(batch, k, j, wdtype="f32"):
    """fp32 tensors (W, W_t rounded to wdtype): activations of order 1, weights of order 1 / sqrt(in), an output
    gradient with a mean (so that the bias gradient does not cancel), non-zero dW / db to accumulate into."""
    g = _gen(batch, k, j)
    r = lambda *s: torch.randn(*s, generator=g)
    rw = lambda *s: (torch.randn(*s, generator=g) / k ** 0.5).to(storage(wdtype)).float()
    d = dict(x=r(batch, k), x_t=r(batch, k), W=rw(j, k), W_t=rw(j, k), b=r(j), b_t=r(j), dy=r(batch, j) + 0.25,
             dy_t=r(batch, j) + 0.25, relu_of=F.relu(r(batch, k)), dW0=r(j, k), db0=r(j))
    return d


def pool_inputs(dtype, n, hw, c):
    """activations rounded to the storage type (returned as fp32), [n, c] operands fp32"""
    g = _gen(n, hw, c, dtype == "bf16")
    st = storage(dtype)
    ra = lambda: torch.randn(n, hw, c, generator=g).to(st).float()
    rv = lambda: torch.randn(n, c, generator=g)
    return dict(a=ra(), a_t=ra(), b=ra(), b_t=ra(), gate=torch.sigmoid(rv()), gate_t=0.3 * rv(), ybar=rv(), ybar_t=rv())


def avgpool_inputs(dtype, n, h, w, c):
    g = _gen(n, h, w, c, dtype == "bf16", 7)
    st = storage(dtype)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    return dict(x=torch.randn(n, h, w, c, generator=g).to(st).float(),
                dout=torch.randn(n, ho, wo, c, generator=g).to(st).float())


# ------------------------------------------------------------------------------------------------ linear layers
def _d(t, like=None):
    return torch.zeros_like(like, dtype=F64) if t is None else t.to(F64)


def _act(v, act):
    return v if act == 0 else (F.relu(v) if act == 1 else torch.sigmoid(v))


def linear_fwd(x, W, b=None, act=0, alpha=1.0):
    """y [n, j] = act(alpha * x W^T + b)"""
    x, W = _d(x), _d(W)
    return _act(alpha * (x @ W.T) + _d(b, W[:, 0]), act)


def linear_fwd_tangent(y, x, x_t, W, W_t, b_t=None, act=0, alpha=1.0):
    """The kernel's contract: act' comes from the STASHED post-activation y (ReLU: [y > 0]; sigmoid: y (1 - y)), the
    result is act'(y) * (alpha * (x_t W^T + x W_t^T) + b_t); a tangent operand that is None is zero."""
    y, x, W = _d(y), _d(x), _d(W)
    lin = lambda xx, ww, bb: alpha * (xx @ ww.T) + bb
    _, lin_t = jvp(lin, (x, W, torch.zeros_like(W[:, 0])), (_d(x_t, x), _d(W_t, W), _d(b_t, W[:, 0])))
    dact = torch.ones_like(y) if act == 0 else ((y > 0).to(F64) if act == 1 else y * (1 - y))
    return dact * lin_t


def _dgrad(dy, W, relu_of):
    # the layer whose backward this is: z = relu(h) W^T (or h W^T), pulled back at h = relu_of (relu_of > 0 iff h > 0)
    h = torch.ones(dy.shape[0], W.shape[1], dtype=F64) if relu_of is None else relu_of
    f = (lambda hh: hh @ W.T) if relu_of is None else (lambda hh: F.relu(hh) @ W.T)
    return vjp(f, h)[1](dy)[0]


def linear_dgrad(dy, W, relu_of=None):
    """dx [n, k] = dy W, times [relu_of > 0] when given"""
    return _dgrad(_d(dy), _d(W), None if relu_of is None else _d(relu_of))


def linear_dgrad_tangent(dy, dy_t, W, W_t, relu_of=None):
    dy, W = _d(dy), _d(W)
    ro = None if relu_of is None else _d(relu_of)
    return jvp(lambda a, b: _dgrad(a, b, ro), (dy, W), (_d(dy_t, dy), _d(W_t, W)))[1]


def _wgrad(dy, x):
    W0, b0 = torch.zeros(dy.shape[1], x.shape[1], dtype=F64), torch.zeros(dy.shape[1], dtype=F64)
    return vjp(lambda W, b: x @ W.T + b, W0, b0)[1](dy)


def linear_wgrad(dy, x):
    """dW [j, k] = dy^T x, db [j] = the column sums of dy"""
    return _wgrad(_d(dy), _d(x))


def linear_wgrad_tangent(dy, dy_t, x, x_t):
    dy, x = _d(dy), _d(x)
    return jvp(_wgrad, (dy, x), (_d(dy_t, dy), _d(x_t, x)))[1]


# ------------------------------------------------------------------------------------------------ pooled / squeeze-excite
def pool_mean(x):
    return _d(x).mean(1)


def _final_pool(cf, relu):
    return (F.relu(cf) if relu else F.silu(cf)).mean(1)


def final_pool(cf, relu=False):
    return _final_pool(_d(cf), relu)


def final_pool_tangent(cf, cf_t, relu=False):
    return jvp(lambda t: _final_pool(t, relu), (_d(cf),), (_d(cf_t),))[1]


def _final_pool_bwd(cf, ybar, relu):
    return vjp(lambda t: _final_pool(t, relu), cf)[1](ybar)[0]


def final_pool_bwd(cf, ybar, relu=False):
    return _final_pool_bwd(_d(cf), _d(ybar), relu)


def final_pool_bwd_tangent(cf, cf_t, ybar, ybar_t, relu=False):
    return jvp(lambda a, b: _final_pool_bwd(a, b, relu), (_d(cf), _d(ybar)), (_d(cf_t), _d(ybar_t)))[1]


def _se_apply(c3, gate, sc, ga, beta):
    x = c3 * gate[:, None, :] * ga + sc
    return x, beta * F.silu(x)


def se_apply(c3, gate, sc, ga, beta):
    """x' = c3 gate ga + sc, a' = beta silu(x')"""
    return _se_apply(_d(c3), _d(gate), _d(sc), ga, beta)


def se_apply_tangent(c3, c3_t, gate, gate_t, sc, sc_t, ga, beta):
    return jvp(lambda a, g, s: _se_apply(a, g, s, ga, beta), (_d(c3), _d(gate), _d(sc)),
               (_d(c3_t), _d(gate_t), _d(sc_t, sc)))[1]


def _se_gate_grad(xbar, c3, gate, ga):
    c3bar, gbar = vjp(lambda a, g: a * g[:, None, :] * ga, c3, gate)[1](xbar)
    return gbar * gate * (1 - gate), c3bar


def se_gate_grad(xbar, c3, gate, ga):
    """zbar [n, c] = (ga sum_hw xbar c3) gate (1 - gate), c3bar = xbar gate ga"""
    return _se_gate_grad(_d(xbar), _d(c3), _d(gate), ga)


def se_gate_grad_tangent(xbar, xbar_t, c3, c3_t, gate, gate_t, ga):
    return jvp(lambda a, b, g: _se_gate_grad(a, b, g, ga), (_d(xbar), _d(c3), _d(gate)),
               (_d(xbar_t), _d(c3_t), _d(gate_t)))[1]


def _avgpool2(x):      # NHWC
    return F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)


def avgpool2(x):
    return _avgpool2(_d(x))


def avgpool2_bwd(dout, h, w):
    dout = _d(dout)
    x0 = torch.zeros(dout.shape[0], h, w, dout.shape[3], dtype=F64)
    return vjp(_avgpool2, x0)[1](dout.contiguous())[0]
