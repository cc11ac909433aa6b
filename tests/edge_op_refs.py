"""Float64 references of the kernels at the edges of every pass -- image_syn -> the first activation tensor and the first
layer's data gradient -> grad_image_syn (csrc/elementwise.hip k_img_gather / k_img_scatter / k_stem_dgrad_image,
csrc/vit.hip k_patchify / k_unpatchify_accum, csrc/nfres.hip k_im2col) -- of the ViT's packing and token glue
(k_lin_pack_all, k_vit_embed / _bwd, k_cls_gather / _scatter, k_add2, k_act_to_f32, k_f32_to_act), of the residual sums
without squeeze-excite (k_resid_relu, k_scale, k_resid_silu) and of the reverse sweep's flat kernels (csrc/flat_ops.hip),
with the shapes and the seeded inputs that tests/test_gpu_edge_ops.py runs them at and tests/test_edge_op_refs_cpu.py
checks them at.  Plain torch, float64, on the storage-rounded inputs the kernel is given, so a comparison isolates the
kernel.  Every accumulating kernel here adds without atomics, on the engine's guarantee that the rows of idx are distinct
within a step: only distinct rows are tested."""
from functools import lru_cache

import torch
import torch.nn.functional as F
from torch.func import jvp

from head_ws_refs import F64, _gen, f32, row_err, storage  # noqa: F401  (row_err / storage: re-exported to the tests)

GARBAGE = 32768.0           # large, finite, exact in bf16: what lanes hold that a kernel must not read
N, NQ = 3, 5                # samples of a step, rows of image_syn
IDX = torch.tensor([3, 0, 4])       # distinct, not monotone; rows 1 and 2 of dimage must come back untouched
COEF, MUL = -1.5, 0.625     # exact in fp32, product exact: the reference's factor is the kernel's
DTYPES = ("f32", "bf16")


def rnd(t, dtype):
    """t rounded to the storage type, as fp32: what the kernel reads"""
    return t.to(storage(dtype)).float()


def randn(shape, dtype, *key, scale=1.0):
    return rnd(scale * torch.randn(shape, generator=_gen(*key)), dtype)


def factor(coef, mul):
    """the fp32 factor mul * coef[0] of the accumulating kernels (coef None = 1)"""
    return f32(f32(mul) * (1.0 if coef is None else f32(coef)))


def image_rows(t):
    """[nq, 3, h, w] -> one row per (image, channel, y) line"""
    return t.reshape(-1, t.shape[-1])


def flat_rows(t, width=8):
    """a flat tensor as rows of `width` elements (one bf16 chunk): one wrong chunk is not averaged away"""
    return t.reshape(-1, width)


def scatter_rows(dimage0, idx, add):
    """dimage0 [nq, ...] (fp32) + add [n, ...] at the rows idx (None = the identity), float64"""
    ref = dimage0.double().clone()
    sel = idx if idx is not None else torch.arange(add.shape[0])
    ref[sel] += add.double()
    return ref


# ------------------------------------------------------------------------------------------------ stem data gradient
# k_stem_dgrad_image: a block owns 8 rows x 128 pixels of one image, blocks = n * (s / 8) * ceil(s / 128)
#   s = 8    one 8-row block, one span: lanes 4 .. 63 of both waves are past x >= s; the last row (y = 7, ty = 0) reads
#            source row 4 = ho, which must be zero-filled
#   s = 24   three row blocks: y0 = 8, 16 take patch rows from oy0 = 4, 8
#   s = 136  two spans: in the first, x = 127 takes tap tx = 0 from patch column 64 (dy column 64, which exists: ho = 68);
#            the second span (x0 = 128) is ragged: 8 pixels, patch columns past ho - 64 = 4 are zero-filled
STEM_S = [8, 24, 136]
STEM_COUT = [8, 16]


def stem_plan(s):
    """(row blocks, spans, blocks per image) as launch_stem_dgrad_image computes them"""
    return s >> 3, (s + 127) >> 7, (s >> 3) * ((s + 127) >> 7)


def stem_cases():
    return [(s, cout, dt) for s in STEM_S for cout in STEM_COUT for dt in DTYPES]


@lru_cache(maxsize=None)
def stem_inputs(s, cout, dtype):
    k = (11, s, cout, DTYPES.index(dtype))
    ho = s // 2
    return {
        "dy1": randn((N, cout, ho, ho), dtype, *k, 1), "dy2": randn((N, cout, ho, ho), dtype, *k, 2),
        "w1": randn((cout, 3, 3, 3), dtype, *k, 3, scale=27 ** -0.5), "w2": randn((cout, 3, 3, 3), dtype, *k, 4, scale=27 ** -0.5),
        "dimage0": torch.randn((NQ, 3, s, s), generator=_gen(*k, 5)),
    }


def stem_dgrad(dy, w, s):
    """d/dx of F.conv2d(x, w, None, 2, 1) against dy, x [n, 3, s, s], by autograd in float64"""
    x = torch.zeros(dy.shape[0], 3, s, s, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(x, w.double(), None, 2, 1), x, dy.double())
    return g


def stem_dgrad_taps(dy, w, s, swap_tx=False, clamp_rows=False, drop_col64=False):
    """the same gradient tap by tap, as the kernel's comment states it:
    dx[n, c, y, x] = sum_{ty, tx, co} dy[n, co, (y + 1 - ty) / 2, (x + 1 - tx) / 2] * w[co, c, ty, tx] over the taps whose
    source coordinate is even and inside.  The flags plant a kernel mistake (tests/test_edge_op_refs_cpu.py)."""
    dy, w = dy.double(), w.double()
    ho = s // 2
    dx = torch.zeros(dy.shape[0], 3, s, s, dtype=F64)
    pos = torch.arange(s)
    for ty in range(3):
        oy = (pos + 1 - ty) // 2
        oky = ((pos + 1 - ty) % 2 == 0) & (oy >= 0) & ((oy <= ho) if clamp_rows else (oy < ho))
        for tx in range(3):
            ox = (pos + 1 - tx) // 2
            okx = ((pos + 1 - tx) % 2 == 0) & (ox >= 0) & (ox < ho)
            if drop_col64:
                okx &= ~((ox == 64) & (pos == 127))
            ys, xs = pos[oky], pos[okx]
            src = dy[:, :, oy[oky].clamp(max=ho - 1)][:, :, :, ox[okx]]
            wk = w[:, :, ty, 2 - tx if swap_tx else tx]
            dx[:, :, ys[:, None], xs[None, :]] += torch.einsum("nohw,oc->nchw", src, wk)
    return dx


def stem_ref(s, cout, dtype, two, idx, coef, mul, grad=stem_dgrad):
    i = stem_inputs(s, cout, dtype)
    g = grad(i["dy1"], i["w1"], s)
    if two:
        g = g + grad(i["dy2"], i["w2"], s)
    return scatter_rows(i["dimage0"], idx, factor(coef, mul) * g)


def pack_dgrad(w, groups=1):
    """tests/test_gpu_ops.py pack_dgrad: OIHW -> [groups][cin_g][k * k][cout_g]"""
    cout, cin_g, k, _ = w.shape
    cout_g = cout // groups
    return w.view(groups, cout_g, cin_g, k, k).permute(0, 2, 3, 4, 1).reshape(groups, cin_g, k * k, cout_g).contiguous()


def pack_fwd(w):
    """tests/test_gpu_ops.py pack_fwd: OIHW -> [cout][k * k][cin_g]"""
    cout, cin_g, k, _ = w.shape
    return w.permute(0, 2, 3, 1).reshape(cout, k * k, cin_g).contiguous()


def stem_wt(w, cin_pad=8):
    """the packed data-gradient weight [cin_pad][9][cout]; the lanes of the padded input channels hold garbage"""
    wt = torch.full((cin_pad, 9, w.shape[0]), GARBAGE)
    wt[:3] = pack_dgrad(w)[0]
    return wt


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ gather / scatter
# (h, w): k_img_gather / k_img_scatter walk n * h * w pixels with 256-thread blocks
#   (8, 8)    192 pixels: one block, its last 64 threads idle
#   (24, 24)  1728 pixels: 7 blocks, the last one ragged (1728 = 6 * 256 + 192)
#   (6, 10)   h != w (a swapped stride shows), 180 pixels
GS_HW = [(8, 8), (24, 24), (6, 10)]
CPAD = 8


@lru_cache(maxsize=None)
def gs_inputs(h, w, dtype):
    k = (12, h, w, DTYPES.index(dtype))
    x0bar = randn((N, h, w, CPAD), dtype, *k, 2)
    x0bar[..., 3:] = GARBAGE                      # the padded channels: never read
    return {"image": torch.randn((NQ, 3, h, w), generator=_gen(*k, 1)), "x0bar": x0bar,
            "dimage0": torch.randn((NQ, 3, h, w), generator=_gen(*k, 3))}


def gather_ref(image, idx, cpad=CPAD):
    """NHWC [n, h, w, cpad] of image[idx] (fp32 values; the caller rounds to the storage type), channels 3.. +0"""
    src = image[idx] if idx is not None else image[:N]
    out = torch.zeros(src.shape[0], src.shape[2], src.shape[3], cpad)
    out[..., :3] = src.permute(0, 2, 3, 1)
    return out


def scatter_ref(dimage0, x0bar, idx, coef, mul):
    return scatter_rows(dimage0, idx, factor(coef, mul) * x0bar[..., :3].permute(0, 3, 1, 2).double())


# ------------------------------------------------------------------------------------------------ patches
# (s, p): (16, 8) a 2 x 2 grid, 768 elements per image; (32, 16) 2 x 2 with the ViT-B patch; (24, 8) a 3 x 3 grid (odd)
PATCH_SP = [(16, 8), (32, 16), (24, 8)]


@lru_cache(maxsize=None)
def patch_inputs(s, p, dtype):
    k = (13, s, p, DTYPES.index(dtype))
    rows, kk = N * (s // p) ** 2, 3 * p * p
    return {"image": torch.randn((NQ, 3, s, s), generator=_gen(*k, 1)), "colsbar": randn((rows, kk), dtype, *k, 2),
            "dimage0": torch.randn((NQ, 3, s, s), generator=_gen(*k, 3))}


def patchify_ref(image, idx, p):
    """[n * (s/p)^2, 3 p p] by F.unfold: row (r, py, px), column c * p * p + dy * p + dx"""
    src = image[idx] if idx is not None else image[:N]
    return F.unfold(src.double(), p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p)


def patchify_index(image, idx, p, swap=False):
    """the same by the explicit index formula (swap: dx and dy exchanged, a planted mistake)"""
    src = (image[idx] if idx is not None else image[:N]).double()
    n, _, s, _ = src.shape
    g = s // p
    r, k = torch.arange(n * g * g)[:, None], torch.arange(3 * p * p)[None, :]
    ni, py, px = r // (g * g), (r // g) % g, r % g
    c, dy, dx = k // (p * p), (k // p) % p, k % p
    if swap:
        dy, dx = dx, dy
    return src[ni, c, py * p + dy, px * p + dx]


def unpatchify_ref(dimage0, colsbar, idx, coef, mul, s, p):
    n = colsbar.shape[0] // (s // p) ** 2
    img = F.fold(colsbar.double().view(n, -1, 3 * p * p).transpose(1, 2), (s, s), p, stride=p)
    return scatter_rows(dimage0, idx, factor(coef, mul) * img)


# ------------------------------------------------------------------------------------------------ im2col
# (h, w, k, stride, pad, cpad); cpad 8 is one chunk in bf16 (cch 1) and two in fp32 (cch 2)
#   (13, 9, 7, 2, 3, 8)   h != w, both odd: ho 7, wo 5; every border has taps outside
#   (16, 16, 7, 2, 3, 8)  the NF-ResNet stem's geometry: wo * 49 * cch = 392 / 784 items per row, more than one trip of 256
#   (10, 10, 3, 1, 1, 8)  stride 1, 3 x 3
IM2COL = [(13, 9, 7, 2, 3, 8), (16, 16, 7, 2, 3, 8), (10, 10, 3, 1, 1, 8)]
IM2COL_N = 2


def im2col_out(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


@lru_cache(maxsize=None)
def im2col_input(case, dtype):
    h, w, k, stride, pad, cpad = case
    return randn((IM2COL_N, h, w, cpad), dtype, 14, *case, DTYPES.index(dtype))


def im2col_ref(x, k, stride, pad):
    """x NHWC -> [n * ho * wo, k * k * cpad] by F.unfold (whose K order is c * k * k + tap), reordered to tap * cpad + c"""
    n, _, _, cpad = x.shape
    u = F.unfold(x.double().permute(0, 3, 1, 2), k, padding=pad, stride=stride)        # [n, cpad * k * k, L]
    return u.view(n, cpad, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * cpad)


def im2col_index(x, k, stride, pad, tx_major=False, pad_used=None):
    """the same by the explicit index formula: column tap * cpad + c, tap = ty * k + tx (tx_major, pad_used: planted mistakes)"""
    x = x.double()
    n, h, w, cpad = x.shape
    ho, wo = im2col_out(h, w, k, stride, pad)
    pad = pad if pad_used is None else pad_used
    m, col = torch.arange(n * ho * wo)[:, None], torch.arange(k * k * cpad)[None, :]
    ni, oy, ox = m // (ho * wo), (m // wo) % ho, m % wo
    tap, c = col // cpad, col % cpad
    ty, tx = (tap % k, tap // k) if tx_major else (tap // k, tap % k)
    iy, ix = oy * stride - pad + ty, ox * stride - pad + tx
    ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    return torch.where(ok, x[ni, iy.clamp(0, h - 1), ix.clamp(0, w - 1), c], torch.zeros((), dtype=F64))


# ------------------------------------------------------------------------------------------------ linear packing
# {out, in} per linear; k_lin_pack_all moves pairs of elements when `in` (wf) / `out` (wt) and the offsets are even
LP_LAUNCHES = {
    # a vit_micro-like layer set (qkv, proj, fc1, fc2 at D = 64), then two layers with ragged 64-tiles in both directions:
    # (72, 40) 2 x 1 tiles (8 rows, 40 columns used), (40, 200) 1 x 4 tiles (the last 8 columns wide).  All offsets even:
    # the paired path throughout
    "vit": [(192, 64), (64, 64), (256, 64), (64, 256), (72, 40), (40, 200)],
    # `in` odd in the first two layers: the scalar fallback for wf, and for wt of (33, 7) and (5, 9) (`out` odd).  off_p
    # turns odd after the first layer (231) and even again after the second (276); off_w stays even (264, 314), so the
    # (64, 64) layer is back on the paired path at a non-zero offset.  The engine cannot reach the fallback: its D is a
    # multiple of the 16-byte chunk, so every `in`, `out` and offset is even
    "odd": [(33, 7), (5, 9), (64, 64)],
    # even `in` and `out` at ODD offsets (off_p = 15): the fallback taken because of the alignment alone
    "odd_offset": [(3, 5), (64, 64)],
}


def lp_descs(shapes):
    """(off_w, off_p, out, in, tile_start) per linear and the tile total, as lin_pack_desc (csrc/vit.hip) builds them"""
    descs, off_w, off_p, tiles = [], 0, 0, 0
    for out, inn in shapes:
        descs.append((off_w, off_p, out, inn, tiles))
        off_w += out * inn + out
        off_p += out * inn
        tiles += ((inn + 63) // 64) * ((out + 63) // 64)
    return descs, tiles, off_w, off_p


def lp_paired(desc):
    """(wf pairs, wt pairs): whether k_lin_pack_all takes the 8-byte path for this layer"""
    off_w, off_p, out, inn, _ = desc
    return inn % 2 == 0 and off_w % 2 == 0 and off_p % 2 == 0, out % 2 == 0 and off_p % 2 == 0


@lru_cache(maxsize=None)
def lp_theta(launch, tangent=False):
    """theta of the launch: per linear the weight, then a bias of NaN (never read)"""
    parts = []
    for li, (out, inn) in enumerate(LP_LAUNCHES[launch]):
        parts += [torch.randn(out * inn, generator=_gen(15, list(LP_LAUNCHES).index(launch), li, int(tangent))),
                  torch.full((out,), float("nan"))]
    return torch.cat(parts)


def lp_refs(launch, tangent=False, untransposed_tile=False):
    """(wf, wt) float64, each the concatenation over the linears (untransposed_tile: a planted mistake in layer (72, 40))"""
    th, wf, wt = lp_theta(launch, tangent).double(), [], []
    for off_w, _, out, inn, _ in lp_descs(LP_LAUNCHES[launch])[0]:
        w = th[off_w:off_w + out * inn].view(out, inn)
        t = w.t().contiguous()
        if untransposed_tile and (out, inn) == (72, 40):
            t[:, 64:] = w.reshape(inn, out)[:, 64:]
        wf.append(w.flatten()), wt.append(t.flatten())
    return torch.cat(wf), torch.cat(wt)


def lp_rows(packed, shapes, which):
    """the rows of a packed buffer: the output channels of wf / the input channels of wt of every linear, as a list"""
    rows = []
    for _, off_p, out, inn, _ in lp_descs(shapes)[0]:
        rows.append(packed[off_p:off_p + out * inn].view((out, inn) if which == "wf" else (inn, out)))
    return rows


# ------------------------------------------------------------------------------------------------ ViT token glue
# (n, tok, dim): (3, 5, 64) a 2 x 2 patch grid; (2, 17, 192) 4 x 4 at ViT-tiny's width; (1, 197, 64) ViT-B's token count,
# one image (dpos = that image's rows), 12608 elements = 50 blocks of the flat kernels, 197 of k_vit_embed_bwd
GLUE = [(3, 5, 64), (2, 17, 192), (1, 197, 64)]


@lru_cache(maxsize=None)
def glue_inputs(n, tok, dim, dtype):
    k = (16, n, tok, dim, DTYPES.index(dtype))
    r = lambda shape, j, rounded=True: randn(shape, dtype, *k, j) if rounded else torch.randn(shape, generator=_gen(*k, j))
    ties = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), 3e38, -0.0, 0.0, 65280.0])   # bf16 ties (to even: down, up), the top binade, zeros
    f = r((n, tok, dim), 13, rounded=False)
    f.view(-1)[:ties.numel()] = ties
    return {
        "pe": r((n, tok - 1, dim), 1), "pe_t": r((n, tok - 1, dim), 2),
        "cls": r((dim,), 3, False), "cls_t": r((dim,), 4, False), "pos": r((tok, dim), 5, False), "pos_t": r((tok, dim), 6, False),
        "xb": r((n, tok, dim), 7), "xb_t": r((n, tok, dim), 8),
        "a": r((n, tok, dim), 9), "a_t": r((n, tok, dim), 10), "b": r((n, tok, dim), 11), "b_t": r((n, tok, dim), 12),
        "f": f, "c": r((n, dim), 14),
    }


def _embed(pe, cls, pos, pos_shift=False, cls_everywhere=False):
    n = pe.shape[0]
    x = torch.cat([cls.expand(n, 1, -1), pe], dim=1)
    if cls_everywhere:
        x = x + torch.cat([torch.zeros_like(cls).expand(n, 1, -1), cls.expand(n, pe.shape[1], -1)], dim=1)
    return x + (pos.roll(1, 0) if pos_shift else pos)


def embed(pe, cls, pos, **mistake):
    return _embed(pe.double(), cls.double(), pos.double(), **mistake)


def embed_tangent(pe, pe_t, cls, cls_t, pos, pos_t):
    d = lambda *t: tuple(v.double() for v in t)
    return jvp(_embed, d(pe, cls, pos), d(pe_t, cls_t, pos_t))[1]


def embed_bwd(xb, dpos_last_only=False, dcls_token1=False):
    """(pebar, dpos, dcls [1, dim]) of the token assembly's backward"""
    xb = xb.double()
    dpos = xb[-1] if dpos_last_only else xb.sum(0)
    dcls = xb[:, 1 if dcls_token1 else 0].sum(0, keepdim=True)
    return xb[:, 1:], dpos, dcls


def cls_gather(x):
    return x[:, 0]


def cls_scatter(c, tok):
    out = torch.zeros(c.shape[0], tok, c.shape[1], dtype=c.dtype)
    out[:, 0] = c
    return out


# ------------------------------------------------------------------------------------------------ residual sums
# elems: 8 one chunk (two in fp32); 4104 = 513 bf16 chunks (1026 fp32): three / five blocks, the last ragged;
# 8 * 8192 * 256 + 8: grid_of caps the grid at 8192 blocks of 256 threads = 2097152 chunks per trip of the grid-stride
# loop, so 2097153 bf16 chunks are the smallest count whose last chunk is taken on a SECOND trip (by thread 0 of block 0;
# fp32: 4194306 chunks, two full trips and two chunks of a third)
RESID_ELEMS = [8, 4104, 8 * 8192 * 256 + 8]
RESID_GRID_CAP, RESID_BLOCK = 8192, 256
ALPHA, BETA = f32(0.2), f32(1.7)
RESID_CLEAR = 1e-4          # ReLU: the float64 min |x'| of every input set stays above this (asserted on the CPU)


def resid_trips(elems, dtype):
    """trips of the grid-stride loop that the busiest thread makes"""
    chunks = elems // (4 if dtype == "f32" else 8)
    grid = max(1, min((chunks + RESID_BLOCK - 1) // RESID_BLOCK, RESID_GRID_CAP))
    return (chunks + grid * RESID_BLOCK - 1) // (grid * RESID_BLOCK)


@lru_cache(maxsize=6)
def resid_inputs(elems, dtype):
    """c3, sc and their tangents.  x' = ALPHA * c3 + sc is placed at least 0.05 from zero (sc is chosen for a target x' and
    then rounded to the storage type, which moves x' by 2^-8 |sc| < 0.03 at most): no seed could keep 16.8 M Gaussian
    samples 1e-4 away from zero, and ReLU's derivative at x' ~ 0 is not what these tests are about."""
    k = (17, elems, DTYPES.index(dtype))
    c3 = randn((elems,), dtype, *k, 1)
    target = torch.randn(elems, generator=_gen(*k, 2))
    target = torch.where(target >= 0, target + 0.05, target - 0.05)
    sc = rnd((target.double() - ALPHA * c3.double()).float(), dtype)
    return {"c3": c3, "sc": sc, "c3_t": randn((elems,), dtype, *k, 3), "sc_t": randn((elems,), dtype, *k, 4)}


def _act(act):
    return F.relu if act == "relu" else F.silu


def resid(c3, sc, act, alpha=ALPHA, beta=BETA, alpha_on_shortcut=False):
    """(x', a') = (alpha c3 + sc, beta act(x'))"""
    c3, sc = c3.double(), sc.double()
    x = alpha * (c3 + sc) if alpha_on_shortcut else alpha * c3 + sc
    return x, beta * _act(act)(x)


def resid_tangent(c3, c3_t, sc, sc_t, act, alpha=ALPHA, beta=BETA, own_sign=False):
    """(x'_t, a'_t) by torch.func.jvp (own_sign: ReLU's tangent masked by the sign of x'_t, a planted mistake)"""
    d = lambda t: t.double()
    fn = lambda a, b: (alpha * a + b, beta * _act(act)(alpha * a + b))
    (x, _), (x_t, a_t) = jvp(fn, (d(c3), d(sc)), (d(c3_t), d(sc_t)))
    if own_sign:
        a_t = beta * torch.where(x_t > 0, x_t, torch.zeros_like(x_t))
    return x_t, a_t


# ------------------------------------------------------------------------------------------------ flat kernels
# the vector kernels take n >> 2 float4 items with at most 2048 blocks of 256 threads, and the n & 3 tail in block 0:
# 1 and 3 tail only, 4 one item, 1027 items + a tail of 3, 2048 * 256 * 4 + 5 one item (and a tail of 1) past a full grid
FLAT_N = [1, 3, 4, 1027, 2048 * 256 * 4 + 5]
D2F_N = [1, 3, 64]           # k_d2f: one wave, i < n


@lru_cache(maxsize=2)
def flat_inputs(n):
    """a, b with <a, b> ~ n / 2 (b = a / 2 + noise: the sum does not cancel, so an error relative to it is meaningful),
    dist0 and the four sums of k_match_finalize"""
    a = torch.randn(n, generator=_gen(18, n, 1))
    b = (0.5 * a + torch.randn(n, generator=_gen(18, n, 2))).float()
    return {"a": a, "b": b, "y0": torch.randn(n, generator=_gen(18, n, 3)),
            "dist0": torch.tensor([3.7], dtype=F64), "s4": torch.tensor([1.25, 3.7, 0.4, 9.1], dtype=F64),
            "acc0": torch.tensor([-7.5], dtype=F64), "d": torch.randn(64, generator=_gen(18, n, 4)).double() * 1e3,
            "out0": torch.randn(64, generator=_gen(18, n, 5))}


def lambda_init(thK, tgt, dist0, two=2.0):
    return (two / float(dist0)) * (thK.double() - tgt.double())


def match_finalize(s4):
    il, tl = s4[0] / s4[1], s4[2] / s4[3]
    return torch.stack([il + tl, il, tl])
