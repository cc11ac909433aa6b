"""Flat parameter vectors of the committed goldens that are regenerated from the golden's seeds instead of being
stored (in full they would put the fixtures over the repository's 1 MiB file limit).  The constructions are the
ones oracle/gen_golden.py uses; each regenerated vector is checked against the fingerprint the golden keeps
(every 97th element, bit for bit, and the float64 sum), so a test never runs on inputs other than the golden's."""
import torch

from oracle import distill_ref as dr
from oracle import nfnet_ref as nr

FINGERPRINT_STRIDE = 97     # oracle/gen_golden.py


def _checked(g, key, t):
    t = t.detach().float().contiguous()
    flat = t.reshape(-1)
    assert torch.equal(flat[::FINGERPRINT_STRIDE], torch.from_numpy(g[key + "_sample"])), \
        "%s regenerated from the golden's seed differs from the golden's" % key
    s, want = flat.double().sum().item(), float(g[key + "_sum"])
    assert abs(s - want) <= 1e-9 * max(1.0, abs(want)), (key, s, want)
    return t


def unroll_params(g):
    """(theta0_img, theta0_txt, target_img, target_txt) of an unroll golden written with full=True
    (gen_golden.gen_unroll / build_pair): CPU float32."""
    seed, d_txt = int(g["seed"]), int(g["d_txt"])
    torch.manual_seed(seed)
    enc = nr.ImageEncoder(str(g["variant"]))
    nr.randomize_like_trained(enc, seed + 1)
    head = dr.ProjectionHead(d_txt, enc.model.num_features)     # same RNG draws as the reference's
    th0i, th0t = dr.FlatModule(enc).flat_param(), dr.FlatModule(head).flat_param()
    gen = torch.Generator().manual_seed(seed + 2)
    tgi = th0i + float(g["sig_img"]) * torch.randn(th0i.shape, generator=gen)
    tgt = th0t + float(g["sig_txt"]) * torch.randn(th0t.shape, generator=gen)
    return (_checked(g, "theta0_img", th0i), _checked(g, "theta0_txt", th0t),
            _checked(g, "target_img", tgi), _checked(g, "target_txt", tgt))


def text_only_theta0(g):
    """theta0 of tests/golden/text_only_unroll.npz (gen_golden.gen_text_only): the projection head built under
    the golden's seed with its LayerNorm weight and bias offset by 0.1 * N(0, 1)."""
    d_out = int(g["d_out"])
    torch.manual_seed(int(g["seed"]))
    head = dr.ProjectionHead(int(g["d_in"]), d_out)
    with torch.no_grad():
        head.layer_norm.weight.add_(0.1 * torch.randn(d_out))
        head.layer_norm.bias.add_(0.1 * torch.randn(d_out))
    return _checked(g, "theta0", dr.FlatModule(head).flat_param())


def reparam_shapes(g, tag):
    """The parameter shapes tests/golden/reparam_reference.npz records, as a list of tuples."""
    dims, out, i = g[tag + "_shape_dims"].tolist(), [], 0
    for nd in g[tag + "_shape_ndim"].tolist():
        out.append(tuple(dims[i:i + nd]))
        i += nd
    return out


def reparam_infos(g, tag):
    return tuple((str(m), str(n)) for m, n in zip(g[tag + "_info_module"], g[tag + "_info_name"]))

