"""The squeeze-excite apply in conv3's forward epilogue (mdd_set_se_fused) against the separate elementwise kernel it
replaces, on the NFNet-l0 topology: mdd_set_se_fused(1), the default = the gate, the residual add and the next
pre-activation are applied by conv3's epilogue; (0) = by k_se_apply_tiled after conv3 has written C3."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

# layer-by-layer f32 bound of the project (DESIGN.md sections 3, 4: f32 buffers agree with the oracle to <= 2e-6)
F32_LAYER_TOL = 2e-6


def _lib():
    from multimodal_dataset_distillation_amd import _lib
    return _lib.load()


class se_mode:
    """process-wide switch, restored on exit"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = _lib().mdd_set_se_fused(self.mode)

    def __exit__(self, *a):
        _lib().mdd_set_se_fused(self.prev)


def _nblocks(eng):
    b = 0
    while True:
        try:
            eng.buffer(f"b{b}.C3", 0)
        except Exception:
            return b
        b += 1


def _theta(eng, seed):
    from multimodal_dataset_distillation_amd.networks import synthetic_expert_params
    return synthetic_expert_params(eng, seed=seed, device=eng.device)


def _assert_fused_kernel_runs(eng, th, img, nb):
    """The comparisons below would pass vacuously if the engine fell back to the separate kernel with the switch on.
    The contraction profile counts the bytes of every conv launch from its epilogue operands: with the apply fused, conv3
    of block b also reads the shortcut and writes X' and (all but the last block) A', i.e. 3 (2) more tensors of C3's
    size in the 128 x 128 class, over the same number of launches."""
    import ctypes as C
    lib = _lib()
    esz = eng.buffer("b0.C3", 0).element_size()
    extra = sum(eng.buffer(f"b{b}.C3", 0).numel() * (3 if b + 1 < nb else 2) for b in range(nb)) * esz
    got = {}
    for mode in (1, 0):
        with se_mode(mode):
            lib.mdd_engine_profile(eng.h, 1)
            eng.img_forward(0, th, img)
            torch.cuda.synchronize()
            buf = (C.c_double * 4)()
            assert lib.mdd_engine_profile_read(eng.h, 2, buf) == 0
            got[mode] = (buf[0], buf[3])
            lib.mdd_engine_profile(eng.h, 0)
    assert got[1][0] == got[0][0] and got[1][1] - got[0][1] == extra, (got, extra)


def test_default_is_fused():
    lib = _lib()
    prev = lib.mdd_set_se_fused(1)
    try:
        assert prev == 1
        assert lib.mdd_set_se_fused(0) == 1 and lib.mdd_set_se_fused(1) == 0
    finally:
        lib.mdd_set_se_fused(prev)


@pytest.mark.parametrize("batch,size", [(4, 224), (3, 96)])
def test_f32_block_buffers_fused_against_unfused(batch, size, report):
    """Every block's X', A' and C3 (primal after mdd_img_forward, tangents after mdd_img_tangent_forward), conv3 epilogue
    against the separate kernel, f32 engine: the same arithmetic on the same stored C3, so at most last-place effects
    may differ (bound: the project's layer-by-layer f32 tolerance).  Measured on the MI355X: all 72 buffers are
    bit-equal (the epilogue places its multiply-adds where this compiler places them in the elementwise kernel; before
    that the tangent buffers differed by up to 1.3e-6).  The number of differing buffers is reported, not asserted: which
    products a compiler contracts is its choice per kernel.  (3, 96): 9 pixels per image in the last stage, so a
    128-row tile spans many images and the last tile is partial."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    eng = UnrollEngine("nfnet_l0", batch=batch, num_queries=batch, image_size=size, d_txt=32, syn_steps=1, dtype="f32")
    th, _ = _theta(eng, 11)
    g = torch.Generator().manual_seed(5)
    img = torch.randn(batch, 3, size, size, generator=g).to(eng.device)
    v = (torch.randn(eng.P_img, generator=g) * float(th.abs().mean())).to(eng.device)
    nb = _nblocks(eng)
    assert nb == 12
    _assert_fused_kernel_runs(eng, th, img, nb)
    got = {}
    for mode in (1, 0):
        with se_mode(mode):
            y = eng.img_forward(0, th, img)
            yd = eng.img_tangent_forward(0, th, v)
            torch.cuda.synchronize()
            bufs = {"y": y.clone(), "y_t": yd.clone()}
            for slot, tag in ((0, ""), (-1, "_t")):
                for b in range(nb):
                    bufs[f"b{b}.C3{tag}"] = eng.buffer(f"b{b}.C3", slot).clone()
                    bufs[f"X{b + 1}{tag}"] = eng.buffer(f"X{b + 1}", slot).clone()
                    if b + 1 < nb:
                        bufs[f"A{b + 1}{tag}"] = eng.buffer(f"A{b + 1}", slot).clone()
            got[mode] = bufs
    worst, worst_name, nbits = 0.0, "", 0
    for k, ref in got[0].items():
        assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0, k
        e = rel_err(got[1][k], ref)
        nbits += int(not torch.equal(got[1][k], ref))
        if e > worst:
            worst, worst_name = e, k
    report(f"se_fused f32 buffers n={batch} s={size}: worst {worst:.2e} ({worst_name}); "
           f"{nbits}/{len(got[0])} buffers differ in some bit")
    eng.close()
    assert worst <= F32_LAYER_TOL, (worst_name, worst)


def _iteration_inputs(eng32, n, size, d_txt, K):
    from multimodal_dataset_distillation_amd.networks import student_move_normalised_targets
    dev = eng32.device
    g = torch.Generator().manual_seed(0)
    image_syn = torch.randn(n, 3, size, size, generator=g).to(dev)
    text_syn = (torch.randn(n, d_txt, generator=g) * 0.5253).to(dev)
    lr = torch.tensor([0.1, 0.1], device=dev)
    th0i, th0t = _theta(eng32, 100)
    gt = torch.Generator(device=dev).manual_seed(200)
    tgi, tgt, _, _ = student_move_normalised_targets(eng32, th0i, th0t, image_syn, text_syn, lr, K, gt)
    perms = torch.stack([torch.randperm(n, generator=g) for _ in range(K)]).to(dev)
    return image_syn, text_syn, lr, th0i, th0t, tgi, tgt, perms


def _match(eng, inp):
    image_syn, text_syn, lr, th0i, th0t, tgi, tgt, perms = inp
    out = eng.unrolled_match(image_syn, text_syn, lr[0:1], lr[1:2], th0i, th0t, tgi, tgt, perms=perms)
    torch.cuda.synchronize()
    return dict(grand=out["grand_loss"].reshape(1).clone(), g_img=out["image_syn"].clone(),
                g_txt=out["text_syn"].clone(), g_lr=out["lr"].clone())


# fused-vs-unfused difference of one bf16 iteration: 2x the largest of five measurements on the MI355X (the project's
# convention for measured budgets: bench.py SELFCHECK_BUDGET); grand was measured exactly equal and is asserted so
BF16_FUSED_VS_UNFUSED = {"grand": 0.0, "g_img": 2 * 6.67e-3, "g_txt": 2 * 2.06e-3, "g_lr": 2 * 8.67e-6}


def test_bf16_unrolled_match_fused_against_unfused(report):
    """One whole outer iteration (NFNet-l0, 10 pairs at 224, 2 inner steps) in bf16, conv3 epilogue against the separate
    kernel on the same inputs, both measured against the f32 engine.  The two carry the same bf16 noise; a rounding lost
    by the fusion would show as a larger error of the fused path, which may exceed the unfused path's by at most 10 %.

    Measured on the MI355X (relative, norm-wise; five runs; the same table is in profiles/se_fused_experiments.md):
                fused vs f32             unfused vs f32           fused vs unfused     unfused vs unfused (two runs)
        grand   1.2364e-03 .. 1.2365e-03 the same                 0 (bit-equal)        0
        g_img   3.7164e-02 .. 3.7181e-02 3.7148e-02 .. 3.7166e-02 4.82e-03 .. 6.67e-03 6.66e-03 .. 6.68e-03
        g_txt   2.0252e-02 .. 2.0307e-02 2.0255e-02 .. 2.0294e-02 1.47e-03 .. 2.06e-03 2.01e-03 .. 2.04e-03
        g_lr    2.4772e-03 .. 2.4802e-03 2.4802e-03 .. 2.4875e-03 6.0e-08 .. 8.67e-06  4.27e-06 .. 5.84e-06
    The forward passes give the same bits either way (f32 test above; grand here).  What remains is not the fusion: two
    runs of the UNFUSED path differ from each other by as much as the fused run differs from either, because the
    convolutions' bias gradients are fp32 atomics in arrival order and a last-place change of an inner gradient grows
    through the bf16 tangent passes like any other bf16 rounding (a fifth of either path's distance to the f32 engine)."""
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    n, size, d_txt, K = 10, 224, 768, 2
    e32 = UnrollEngine("nfnet_l0", batch=n, num_queries=n, image_size=size, d_txt=d_txt, syn_steps=K, dtype="f32")
    inp = _iteration_inputs(e32, n, size, d_txt, K)
    ref = _match(e32, inp)
    e32.close()
    del e32
    e16 = UnrollEngine("nfnet_l0", batch=n, num_queries=n, image_size=size, d_txt=d_txt, syn_steps=K, dtype="bf16")
    _assert_fused_kernel_runs(e16, inp[3], inp[0], 12)
    res = {}
    for tag, mode in (("fused", 1), ("unfused", 0), ("unfused2", 0)):
        with se_mode(mode):
            res[tag] = _match(e16, inp)
    e16.close()
    bad = []
    for k in ("grand", "g_img", "g_txt", "g_lr"):
        ef, eu = rel_err(res["fused"][k], ref[k]), rel_err(res["unfused"][k], ref[k])
        d = rel_err(res["fused"][k], res["unfused"][k])
        report(f"se_fused bf16 iteration {k}: fused-vs-f32 {ef:.4e} unfused-vs-f32 {eu:.4e} fused-vs-unfused {d:.4e} "
               f"bit-equal {torch.equal(res['fused'][k], res['unfused'][k])}; unfused run-to-run "
               f"{rel_err(res['unfused2'][k], res['unfused'][k]):.4e}")
        if not ef <= 1.10 * eu:
            bad.append((k, "error against f32", ef, eu))
        if BF16_FUSED_VS_UNFUSED[k] == 0.0:
            if not torch.equal(res["fused"][k], res["unfused"][k]):
                bad.append((k, "fused != unfused", d))
        elif not d <= BF16_FUSED_VS_UNFUSED[k]:
            bad.append((k, "fused vs unfused", d, BF16_FUSED_VS_UNFUSED[k]))
    assert not bad, bad
