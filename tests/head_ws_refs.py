"""Float64 references of weight standardisation (csrc/ws.hip), of the text head's pointwise / LayerNorm / row kernels and
of the contrastive head (csrc/head.hip), with the shapes and the seeded inputs that tests/test_gpu_head_ws.py runs them at
and tests/test_head_ws_refs_cpu.py checks them at.  Plain torch: tangents through torch.func.jvp, backward passes through
torch.func.vjp, the tangent of a backward pass as the jvp of that vjp.  Every function computes in float64 whatever it is
given; the inputs are fp32 tensors (theta, the gradients and the head's activations are fp32 in the engine), so a
comparison isolates the kernel."""
import math
from functools import lru_cache

import torch
import torch.nn.functional as F
from torch.func import jvp, vjp

F64 = torch.float64


def _d(t):
    return t.to(F64)


def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1000003 + int(v)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def storage(dtype):
    return torch.float32 if dtype == "f32" else torch.bfloat16


def f32(v):
    """the value a C float argument takes: the references use what the kernel is given"""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ error measures
def row_err(got, ref):
    """the maximum over rows (dim 0) of |got_row - ref_row| / |ref_row|: one wrong output channel / sample is not
    averaged away by the others.  A row whose reference is exactly zero counts with its absolute error."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    den = ref.norm(dim=1)
    e = (got - ref).norm(dim=1) / torch.where(den > 0, den, torch.ones_like(den))
    return float(torch.nan_to_num(e, nan=float("inf")).max())


def elem_err(got, ref):
    """the largest element error, absolute where the reference stays below 1 and relative to its largest element above
    (column sums over n rows, scalars, the loss)"""
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = (got - ref).abs().max() / max(1.0, float(ref.abs().max()))
    return float(torch.nan_to_num(e, nan=float("inf")))


def scalar_err(got, ref):
    """relative error of a scalar (absolute where the reference is exactly zero)"""
    got, ref = float(got), float(ref)
    e = abs(got - ref) / (abs(ref) if ref != 0 else 1.0)
    return e if e == e else float("inf")


def gain_err(got, ref):
    """the gain gradient of a conv, one scalar per output channel (a sum of fan products that may cancel): the largest
    element error against the root mean square of the conv's gain gradients"""
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = (got - ref).abs().max() / ref.pow(2).mean().sqrt()
    return float(torch.nan_to_num(e, nan=float("inf")))


# ------------------------------------------------------------------------------------------------ weight standardisation
# csrc/ws.hip: a forward block owns WS_TILE_ROWS output channels of one group and streams them WS_SLAB weights at a
# time; a wave takes the row statistics WS_STAT_TRIP = 64 lanes x 8 loads at a time
WS_TILE_ROWS, WS_SLAB, WS_STAT_TRIP = 16, 64, 512
WS_GAMMA, WS_EPS = f32(1.7015043497085571), f32(1e-5)     # the SiLU gamma and the eps of timm's ScaledStdConv2d in the NFNets
# (cout, cin, k, groups, cin_pad)
WS_SHAPES = [
    (16, 3, 3, 1, 8),           # (a) fan 27 < one slab; channels padded 3 -> 8
    (24, 16, 3, 1, 16),         # (b) fan 144; tiles of 16 + 8 rows
    (64, 64, 3, 1, 64),         # (c) fan 576 = one full 512-weight statistics trip + 64
    (48, 48, 3, 6, 48),         # (d) 8-channel groups; every tile half empty; fan 72
    (40, 104, 1, 1, 104),       # (e) pointwise; ragged slab; 16 + 16 + 8 rows
    (128, 128, 3, 2, 128),      # (f) 64-wide groups
    (24, 1096, 1, 1, 1096),     # (g) three statistics trips; ragged
]
WS_SMALL_STD = WS_SHAPES[1]     # this conv's weights have std 0.01: eps = 1e-5 is 10 % of their variance
# the launches: all seven (descriptor search, offsets), (b) alone, the list reversed
WS_LAUNCHES = {"all": list(WS_SHAPES), "b_alone": [WS_SHAPES[1]], "reversed": list(reversed(WS_SHAPES))}
WS_PAD_SENTINEL = 7.25          # exact in bf16; what the padded lanes of the packed buffers hold before a forward call


def ws_plan(shape):
    """what a conv is to the kernels of csrc/ws.hip -- restated here so that the properties claimed beside the shapes
    are checked (tests/test_head_ws_refs_cpu.py), not only written down"""
    cout, cin, k, groups, cin_pad = shape
    cin_g, cout_g, cpg = cin // groups, cout // groups, cin_pad // groups
    fan = cin_g * k * k
    tpg = -(-cout_g // WS_TILE_ROWS)
    return dict(fan=fan, cin_g=cin_g, cout_g=cout_g, cin_pad_g=cpg, ksq=k * k, tiles=groups * tpg,
                tile_rows=[min(WS_TILE_ROWS, cout_g - t * WS_TILE_ROWS) for t in range(tpg)],
                slabs=-(-fan // WS_SLAB), last_slab=fan - (-(-fan // WS_SLAB) - 1) * WS_SLAB,
                stat_trips=-(-fan // WS_STAT_TRIP), packed=cout * k * k * cpg, theta=cout * fan + cout)


@lru_cache(maxsize=None)
def ws_conv_inputs(shape):
    """fp32: weights with a mean (so that the mean subtraction matters), gains around 1, the gradient of the
    standardised weights with a mean (so that mean(dwh) does not cancel), and a direction for each.  Seeded by the
    shape: a conv has the same inputs in every launch, and its references are computed once."""
    cout, cin, k, groups, _ = shape
    g = _gen(11, *shape)
    std = 0.01 if shape == WS_SMALL_STD else 1.0
    r = lambda *s: torch.randn(*s, generator=g)
    ws = (cout, cin // groups, k, k)
    return dict(w=(r(*ws) + 0.3) * std, w_t=r(*ws) * std, gain=1 + 0.3 * r(cout), gain_t=r(cout), dwh=r(*ws) + 0.25,
                dwh_t=r(*ws) + 0.25)


def _ws_std(w, gain, gamma, eps):
    cout, fan = w.shape[0], w[0].numel()
    r = w.reshape(cout, fan)
    mu = r.sum(1, keepdim=True) / fan
    var = ((r - mu) ** 2).sum(1, keepdim=True) / fan                  # biased
    return ((r - mu) / torch.sqrt(var + eps) * (gain[:, None] * (gamma / math.sqrt(fan)))).reshape(w.shape)


def ws_std(w, gain, gamma=WS_GAMMA, eps=WS_EPS):
    """w_hat [cout, cin_g, k, k] = gain gamma fan^-1/2 (w - mean) / sqrt(var + eps), per output channel"""
    return _ws_std(_d(w), _d(gain), gamma, eps)


def ws_std_tangent(w, w_t, gain, gain_t, gamma=WS_GAMMA, eps=WS_EPS):
    return jvp(lambda a, b: _ws_std(a, b, gamma, eps), (_d(w), _d(gain)), (_d(w_t), _d(gain_t)))[1]


def _ws_bwd(w, gain, dwh, gamma, eps):
    return vjp(lambda a, b: _ws_std(a, b, gamma, eps), w, gain)[1](dwh)


def ws_bwd(w, gain, dwh, gamma=WS_GAMMA, eps=WS_EPS):
    """(dw, dgain): the vjp of ws_std along dwh"""
    return _ws_bwd(_d(w), _d(gain), _d(dwh), gamma, eps)


def ws_bwd_tangent(w, w_t, gain, gain_t, dwh, dwh_t, gamma=WS_GAMMA, eps=WS_EPS):
    """the jvp of that vjp along (w_t, gain_t, dwh_t)"""
    return jvp(lambda a, b, c: _ws_bwd(a, b, c, gamma, eps), (_d(w), _d(gain), _d(dwh)),
               (_d(w_t), _d(gain_t), _d(dwh_t)))[1]


def pack_wf(wh, shape, fill, dtype=F64):
    """wf [cout][tap][cin_pad_g], by plain indexing; the padded lanes hold `fill`"""
    cout, cin, k, groups, cin_pad = shape
    out = torch.full((cout, k * k, cin_pad // groups), fill, dtype=dtype)
    for ci in range(cin // groups):
        for tap in range(k * k):
            out[:, tap, ci] = wh[:, ci, tap // k, tap % k]
    return out


def pack_wt(wh, shape, fill, dtype=F64):
    """wt [g][cin_pad_g][tap][cout_g], by plain indexing; the padded lanes hold `fill`"""
    cout, cin, k, groups, cin_pad = shape
    cout_g = cout // groups
    out = torch.full((groups, cin_pad // groups, k * k, cout_g), fill, dtype=dtype)
    for g in range(groups):
        for ci in range(cin // groups):
            for tap in range(k * k):
                out[g, ci, tap, :] = wh[g * cout_g:(g + 1) * cout_g, ci, tap // k, tap % k]
    return out


def wf_rows(packed, shape):
    """a packed wf as [cout, everything of that output channel]"""
    return packed.reshape(shape[0], -1)


def wt_rows(packed, shape):
    cout, cin, k, groups, cin_pad = shape
    return packed.reshape(groups, cin_pad // groups, k * k, cout // groups).permute(0, 3, 1, 2).reshape(cout, -1)


@lru_cache(maxsize=None)
def ws_conv_refs(shape):
    """every float64 reference of one conv (shared by the launches and never modified)"""
    i = ws_conv_inputs(shape)
    wh = ws_std(i["w"], i["gain"])
    wh_t = ws_std_tangent(i["w"], i["w_t"], i["gain"], i["gain_t"])
    dw, dgain = ws_bwd(i["w"], i["gain"], i["dwh"])
    dw_t, dgain_t = ws_bwd_tangent(i["w"], i["w_t"], i["gain"], i["gain_t"], i["dwh"], i["dwh_t"])
    S = WS_PAD_SENTINEL
    return dict(wh=wh, wh_t=wh_t, dw=dw, dgain=dgain, dw_t=dw_t, dgain_t=dgain_t,
                wf=pack_wf(wh, shape, S), wt=pack_wt(wh, shape, S), wf_t=pack_wf(wh_t, shape, S),
                wt_t=pack_wt(wh_t, shape, S), pad_wf=torch.isnan(pack_wf(wh, shape, float("nan"))),
                pad_wt=torch.isnan(pack_wt(wh, shape, float("nan"))))


def ws_theta(shapes, wkey="w", gkey="gain"):
    """flat fp32 theta of a launch: per conv the weight OIHW, then the gain"""
    return torch.cat([t.flatten() for s in shapes for t in (ws_conv_inputs(s)[wkey], ws_conv_inputs(s)[gkey])])


def ws_dwf(shapes, key="dwh"):
    """the fp32 gradient of the standardised weights of a launch in the wf layout, NaN in the padded lanes"""
    return torch.cat([pack_wf(ws_conv_inputs(s)[key], s, float("nan"), torch.float32).flatten() for s in shapes])


def ws_offsets(shapes):
    """per conv (theta offset of the weights, of the gains, packed offset)"""
    out, ot, op = [], 0, 0
    for s in shapes:
        p = ws_plan(s)
        out.append((ot, ot + s[0] * p["fan"], op))
        ot, op = ot + p["theta"], op + p["packed"]
    return out, ot, op


# ------------------------------------------------------------------------------------------------ text head
HEAD_N = [1, 3, 100]
HEAD_D = [8, 255, 257, 1000, 2304]
LN_EPS = f32(1e-5)


def head_cases():
    return [(n, d) for n in HEAD_N for d in HEAD_D]


@lru_cache(maxsize=None)
def head_inputs(n, d):
    """fp32.  p covers [-6, 6] and contains 0, -6 and 6; the dropout mask is scaled by 1 / (1 - 0.3) and contains zeros;
    the output gradients have a mean; idx is a permutation of the rows of a table with three spare rows."""
    g = _gen(23, n, d)
    r = lambda *s: torch.randn(*s, generator=g)
    p = torch.rand(n, d, generator=g) * 12 - 6
    p.view(-1)[0], p.view(-1)[1], p.view(-1)[-1] = 0.0, -6.0, 6.0
    mask = (torch.rand(n, d, generator=g) > 0.3).float() / 0.7
    mask.view(-1)[0] = 0.0
    rows = n + 3
    return dict(p=p, p_t=r(n, d), rbar=r(n, d), rbar_t=r(n, d), gbar=r(n, d) + 0.25, gbar_t=r(n, d), f=r(n, d), f_t=r(n, d),
                q=r(n, d) + 0.2, q_t=r(n, d), mask=mask, gamma=1 + 0.3 * r(d), gamma_t=r(d), beta=r(d), beta_t=r(d),
                ybar=r(n, d) + 0.25, ybar_t=r(n, d) + 0.25, table=r(rows, d), acc0=r(rows, d),
                idx=torch.randperm(rows, generator=g)[:n], coef=torch.tensor([0.37]))


def _gelu(p):
    return 0.5 * p * (1 + torch.erf(p / math.sqrt(2.0)))


def gelu(p):
    return _gelu(_d(p))


def gelu_tangent(p, p_t):
    return jvp(_gelu, (_d(p),), (_d(p_t),))[1]


def _gelu_bwd(p, rbar, gbar):
    return rbar + vjp(_gelu, p)[1](gbar)[0]


def gelu_bwd(p, rbar, gbar):
    """pbar = rbar + gbar GELU'(p)"""
    return _gelu_bwd(_d(p), _d(rbar), _d(gbar))


def gelu_bwd_tangent(p, p_t, rbar, rbar_t, gbar, gbar_t):
    return jvp(_gelu_bwd, (_d(p), _d(rbar), _d(gbar)), (_d(p_t), _d(rbar_t), _d(gbar_t)))[1]


def _ln(r, gamma, beta, eps):
    mu = r.mean(1, keepdim=True)
    var = ((r - mu) ** 2).mean(1, keepdim=True)
    return (r - mu) / torch.sqrt(var + eps) * gamma + beta


def _ln_fwd(f, p, gamma, beta, mask, eps):
    r = f * mask + p if mask is not None else f + p
    return _ln(r, gamma, beta, eps), r


def _m(mask):
    return None if mask is None else _d(mask)


def _z(t, like):
    return torch.zeros_like(like, dtype=F64) if t is None else _d(t)


def ln_fwd(f, p, gamma, beta, mask=None, eps=LN_EPS):
    """(y, r): r = f mask + p, y = LayerNorm(r) gamma + beta"""
    return _ln_fwd(_d(f), _d(p), _d(gamma), _d(beta), _m(mask), eps)


def ln_fwd_tangent(f, f_t, p, p_t, gamma, gamma_t, beta, beta_t, mask=None, eps=LN_EPS):
    """(y_t, r_t); gamma_t / beta_t None = 0"""
    mk = _m(mask)
    return jvp(lambda a, b, c, e: _ln_fwd(a, b, c, e, mk, eps), (_d(f), _d(p), _d(gamma), _d(beta)),
               (_d(f_t), _d(p_t), _z(gamma_t, gamma), _z(beta_t, beta)))[1]


def _ln_bwd(ybar, r, gamma, mask, eps):
    rbar, dgamma, dbeta = vjp(lambda a, b, c: _ln(a, b, c, eps), r, gamma, torch.zeros_like(gamma))[1](ybar)
    return rbar, (rbar * mask if mask is not None else rbar), dgamma, dbeta


def ln_bwd(ybar, r, gamma, mask=None, eps=LN_EPS):
    """(rbar, fbar = rbar mask, dgamma, dbeta) of y = LayerNorm(r) gamma + beta along ybar"""
    return _ln_bwd(_d(ybar), _d(r), _d(gamma), _m(mask), eps)


def ln_bwd_tangent(ybar, ybar_t, r, r_t, gamma, gamma_t, mask=None, eps=LN_EPS):
    mk = _m(mask)
    return jvp(lambda a, b, c: _ln_bwd(a, b, c, mk, eps), (_d(ybar), _d(r), _d(gamma)),
               (_d(ybar_t), _d(r_t), _z(gamma_t, gamma)))[1]


# ------------------------------------------------------------------------------------------------ contrastive head
CON_SHAPES = [(1, 8), (2, 64), (3, 4096), (5, 257), (67, 1000), (130, 2304)]
CON_SCALES_DEV = [0.1, 0.7, -0.5, 1 / 0.07]     # through the device scalar; 0.7 also through scale_const
CON_HOT = 1 / 0.07
# what an fp32 torch evaluation of the same formula (oracle.distill_ref.contrastive_loss, torch.autograd) reaches against
# these references on these inputs, per row, over all shapes and quantities: measured on the CPU, asserted by
# tests/test_head_ws_refs_cpu.py
TORCH_F32_ERR = {"unit": 5e-7, "hot": 1.1e-5}   # |scale| <= 1 ; scale 1 / 0.07
TORCH_F32_SCALAR_ERR = 5e-6                     # loss, sbar, sbar_t: relative, every scale


@lru_cache(maxsize=None)
def con_inputs(n, d):
    """y = 0.5 x + noise, so that the diagonal of the logits stands out (the symmetric cross-entropy's -2 I matters).
    The seed is one at which no small case saturates at scale 1 / 0.07: with n = 2 some draws put a diagonal probability
    within 1e-3 of 1, P - 1 cancels, and the fp32 torch evaluation itself is off by 1e-4 and more there -- the
    ill-conditioning a saturated scale would bring to every case, which a kernel test must stay away from."""
    g = _gen(60, n, d)
    r = lambda: torch.randn(n, d, generator=g)
    x = r()
    return dict(x=x, y=0.5 * x + r(), x_t=r(), y_t=r())


def _closs(x, y, scale):
    # oracle.distill_ref.contrastive_loss without its .float() (which would take the float64 inputs back to fp32);
    # tests/test_head_ws_refs_cpu.py holds the two together
    x = x / x.norm(dim=1, keepdim=True)
    y = y / y.norm(dim=1, keepdim=True)
    logits = scale * x @ y.t()
    gt = torch.arange(len(logits))
    return (F.cross_entropy(logits, gt) + F.cross_entropy(logits.t(), gt)) / 2


def _cgrad(x, y, scale):
    loss, pull = vjp(_closs, x, y, scale)
    return (loss,) + pull(torch.ones_like(loss))


def _s(scale):
    return torch.as_tensor(scale, dtype=F64)


def contrastive(x, y, scale):
    """(loss, xbar, ybar, sbar)"""
    return _cgrad(_d(x), _d(y), _s(scale))


def contrastive_tangent(x, x_t, y, y_t, scale):
    """the directional derivative of (xbar, ybar, sbar) along (x_t, y_t); the scale has no tangent"""
    s = _s(scale)
    return jvp(lambda a, b: _cgrad(a, b, s)[1:], (_d(x), _d(y)), (_d(x_t), _d(y_t)))[1]


@lru_cache(maxsize=None)
def con_refs(n, d, scale):
    i = con_inputs(n, d)
    scale = f32(scale)
    loss, xbar, ybar, sbar = contrastive(i["x"], i["y"], scale)
    xbar_t, ybar_t, sbar_t = contrastive_tangent(i["x"], i["x_t"], i["y"], i["y_t"], scale)
    return dict(loss=loss, xbar=xbar, ybar=ybar, sbar=sbar, xbar_t=xbar_t, ybar_t=ybar_t, sbar_t=sbar_t)
