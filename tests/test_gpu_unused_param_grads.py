"""mdd_unrolled_match without the parameter gradients nothing reads (mdd_set_skip_unused_param_grads, default 1): the
Hessian-vector product of reverse step 0 and the inner gradient of a recomputed step are not computed.  The switch-off
path is the engine as it was and the yardstick: the outputs with the switch on are compared with it, bounded by the
project's f32 layer bound or twice what switch-off runs differ by among themselves, whichever is larger."""
import ctypes as C

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

# the project's f32 bound (tests/test_gpu_se_fused.py F32_LAYER_TOL) and the bf16 bar of tests/test_gpu_engine.py (TOL["bf16"])
F32_TOL = 2e-6
BF16_TOL = 8e-2
N, SIZE, D_TXT = 4, 64, 16
OUTPUTS = ("losses", "image_syn", "text_syn", "lr")
VARIANTS = ["nfnet_tiny", "nf_resnet_tiny", "nf_regnet_tiny", "vit_micro", "clip_vit_micro"]
# (steps the engine is built for, keep_steps (None = all), syn_steps of the call (None = the engine's))
SWEEPS = {"keep_all": (3, None, None), "keep_0": (3, 0, None), "keep_1": (3, 1, None), "one_step": (1, None, None),
          "fewer_steps": (3, None, 2)}


def _lib():
    from multimodal_dataset_distillation_amd import _lib
    return _lib.load()


class skip_mode:
    """process-wide switch, restored on exit"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = _lib().mdd_set_skip_unused_param_grads(self.mode)

    def __exit__(self, *a):
        _lib().mdd_set_skip_unused_param_grads(self.prev)


def _engine(variant, dtype, K, keep, nq=N):
    from multimodal_dataset_distillation_amd.engine import UnrollEngine
    return UnrollEngine(variant, batch=N, num_queries=nq, image_size=SIZE, d_txt=D_TXT, syn_steps=K, dtype=dtype,
                        keep_steps=keep)


def _inputs(eng, steps, nq=N):
    """as bench.py builds them: a trained-like expert snapshot and targets one student move away (matching loss ~ 4)"""
    from multimodal_dataset_distillation_amd.networks import (student_move_normalised_targets,
                                                               synthetic_expert_params)
    dev = eng.device
    g = torch.Generator().manual_seed(0)
    image_syn = torch.randn(nq, 3, SIZE, SIZE, generator=g).to(dev)
    text_syn = (torch.randn(nq, D_TXT, generator=g) * 0.5253).to(dev)
    lr = torch.tensor([0.1, 0.1], device=dev)
    th0i, th0t = synthetic_expert_params(eng, seed=100, device=dev)
    gt = torch.Generator(device=dev).manual_seed(200)
    tgi, tgt, _, _ = student_move_normalised_targets(eng, th0i, th0t, image_syn, text_syn, lr, steps, gt)
    perms = torch.stack([torch.randperm(nq, generator=g)[:N] for _ in range(steps)]).to(dev)
    return image_syn, text_syn, lr, th0i, th0t, tgi, tgt, perms


def _match(eng, inp, steps):
    image_syn, text_syn, lr, th0i, th0t, tgi, tgt, perms = inp
    out = eng.unrolled_match(image_syn, text_syn, lr[0:1], lr[1:2], th0i, th0t, tgi, tgt, perms=perms, syn_steps=steps)
    torch.cuda.synchronize()
    assert out["losses"].numel() == 3 + steps
    return {k: out[k].clone() for k in OUTPUTS}


_COMPARED = {}


def _compare(variant, dtype, sweep, nq=N):
    """Three iterations with the switch off, two with it on, same engine and inputs; per output the largest difference
    among the switch-off runs and the largest difference of a switch-on run from the first switch-off run."""
    key = (variant, dtype, sweep, nq)
    if key not in _COMPARED:
        K, keep, steps = SWEEPS[sweep]
        steps = K if steps is None else steps
        eng = _engine(variant, dtype, K, keep, nq)
        inp = _inputs(eng, steps, nq)
        with skip_mode(0):
            off = [_match(eng, inp, steps) for _ in range(3)]
        with skip_mode(1):
            on = [_match(eng, inp, steps) for _ in range(2)]
        eng.close()
        res = {}
        for k in OUTPUTS:
            for r in off + on:
                assert torch.isfinite(r[k]).all(), (key, k)
            assert float(off[0][k].abs().max()) > 0, (key, k)
            spread = max(rel_err(off[i][k], off[j][k]) for i, j in ((1, 0), (2, 0), (2, 1)))
            diff = max(rel_err(r[k], off[0][k]) for r in on)
            res[k] = (spread, diff)
        res["grand"] = float(off[0]["losses"][0])
        _COMPARED[key] = res
    return _COMPARED[key]


def _figures(tag, res, report):
    report(f"unused_param_grads {tag}: grand {res['grand']:.3f}; " +
           "; ".join(f"{k} on-vs-off {res[k][1]:.2e} (off run-to-run {res[k][0]:.2e})" for k in OUTPUTS))


def test_switch_default_and_restore():
    lib = _lib()
    prev = lib.mdd_set_skip_unused_param_grads(1)
    try:
        assert prev == 1
        assert lib.mdd_set_skip_unused_param_grads(0) == 1 and lib.mdd_set_skip_unused_param_grads(1) == 0
    finally:
        lib.mdd_set_skip_unused_param_grads(prev)
    assert lib.mdd_set_skip_unused_param_grads(prev) == prev


@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_f32_same_results(variant, sweep, report):
    """The data path with the switch on is the same launches on the same inputs, so the f32 outputs may differ from
    the switch-off ones only as two switch-off runs differ (the fp32-atomic order of the bias and LayerNorm sums).

    Measured on the MI355X (profiles/unused_param_grads_ab.md section 2): in a whole-suite run on-vs-off lies between
    0 and 3.9e-6 where the switch-off runs differ by up to 4.7e-6 among themselves.  Under this bound the test is NOT
    stable, for two reasons that lie in the switch-off path (the yardstick) and that no change on the switch-on side
    removes; the bound, the cases and the inputs are left as they are and the cases below fail now and then:
      * nf_resnet_tiny, K = 3: in about one run of twelve the switch-off path itself gives a second, discrete result,
        image_syn 5.97e-5 and text_syn 3.4e-6 away.  Measured cause: exactly one stashed ReLU mask flips, block 0's conv2
        pre-activation of step 2 is +3.4e-7 in one run and -1.3e-7 in the other (1 of 65536 elements within 5e-7 of
        zero), moved by the arrival order of the fp32 bias-gradient atomics of the earlier steps; no mask differs between
        two runs that agree.  When a switch-on run lands there and none of the three switch-off runs does, the case
        fails: seen for keep_0 and for keep_all (image_syn 5.97e-5, text_syn 3.4e-6 against 2e-6).  Twelve interleaved
        runs per setting show the same two results at the same rate with the switch off and on.
      * vit_micro / clip_vit_micro: their run-to-run spread (the LayerNorm and bias atomics) is 6e-7 .. 5e-6, and three
        switch-off runs that happen to agree to 8e-7 leave a bound of 2e-6: seen for clip_vit_micro keep_all (image_syn
        3.9e-6, text_syn 5.5e-6; other runs of that case: 2.9e-6 / 3.2e-6 on both sides), for clip_vit_micro fewer_steps
        and for vit_micro fewer_steps (image_syn 4.1e-6 where the three switch-off runs agreed to 8.6e-7)."""
    res = _compare(variant, "f32", sweep)
    _figures(f"f32 {variant} {sweep}", res, report)
    bad = [(k, res[k][1], max(F32_TOL, 2 * res[k][0])) for k in OUTPUTS if not res[k][1] <= max(F32_TOL, 2 * res[k][0])]
    assert not bad, bad


def test_f32_lr_gradient_reads_the_forward_sweeps_inner_gradients(report):
    """keep_steps = 0: two of the three steps are recomputed in the reverse sweep.  The learning-rate gradient is
    -sum_k <g_k, lambda>, the only output a zeroed or doubled g_k of a recomputed step would show in."""
    res = _compare("nfnet_tiny", "f32", "keep_0")
    spread, diff = res["lr"]
    report(f"unused_param_grads f32 nfnet_tiny keep_0 lr gradient: on-vs-off {diff:.2e} (off run-to-run {spread:.2e})")
    assert diff <= max(F32_TOL, 2 * spread), \
        f"the recomputed steps changed g_k: lr gradient differs by {diff:.2e} (switch-off runs: {spread:.2e})"


@pytest.mark.parametrize("variant", ["nfnet_tiny", "nf_regnet_tiny"])
def test_f32_recomputed_steps_of_different_minibatches(variant, report):
    """keep_steps = 0 with 4 of 7 pairs drawn per step.  The tangent pass of a step reads the step's own primal packed
    weight gradient (the weight-standardisation backward is differentiated); a recomputed step that does not run its
    weight gradients must find the forward sweep's.  With every step on the same four pairs the packed gradients of two
    steps differ too little for a stale one to show; with different pairs per step it shows at 5e-5."""
    res = _compare(variant, "f32", "keep_0", nq=7)
    _figures(f"f32 {variant} keep_0, 4 of 7 pairs per step", res, report)
    bad = [(k, res[k][1], max(F32_TOL, 2 * res[k][0])) for k in OUTPUTS if not res[k][1] <= max(F32_TOL, 2 * res[k][0])]
    assert not bad, bad


@pytest.mark.parametrize("variant", ["nfnet_tiny", "vit_micro"])
def test_bf16_same_results(variant, report):
    """bf16 iterations are not reproducible to the bit (tests/test_gpu_se_fused.py): the sharp check is the f32 one; here
    the outputs are finite (asserted in _compare) and the two paths agree within the engine's bf16 bar."""
    res = _compare(variant, "bf16", "keep_all")
    _figures(f"bf16 {variant} keep_all", res, report)
    bad = [(k, res[k][1]) for k in OUTPUTS if not res[k][1] <= BF16_TOL]
    assert not bad, bad


def _wgrad_launches(eng, run):
    lib = _lib()
    lib.mdd_engine_profile(eng.h, 1)
    try:
        run()
        torch.cuda.synchronize()
        buf = (C.c_double * 4)()
        assert lib.mdd_engine_profile_read(eng.h, 3, buf) == 0
        return int(buf[0])
    finally:
        lib.mdd_engine_profile(eng.h, 0)


@pytest.mark.parametrize("keep,passes_off,passes_on", [(None, 3 + 0 + 3, 3 + 0 + 2), (0, 3 + 2 + 3, 3 + 0 + 2)])
def test_weight_gradient_launches_are_dropped(keep, passes_off, passes_on):
    """Not vacuous: conv weight-gradient launches (profile kind 3) of one iteration, K = 3, as multiples of one backward
    pass's: forward sweep + recomputed steps + tangent passes."""
    eng = _engine("nfnet_tiny", "f32", 3, keep)
    inp = _inputs(eng, 3)
    y = eng.img_forward(0, inp[3], inp[0])
    n = _wgrad_launches(eng, lambda: eng.img_backward(0, inp[3], torch.ones_like(y)))
    assert n > 0
    got = {}
    for mode in (0, 1):
        with skip_mode(mode):
            got[mode] = _wgrad_launches(eng, lambda: _match(eng, inp, 3))
    eng.close()
    assert got == {0: passes_off * n, 1: passes_on * n}, (got, n)


def test_op_level_passes_keep_their_parameter_gradients(report):
    """The mode does not outlive mdd_unrolled_match: the op-level tangent backward passes return the same non-zero H v
    before and after an iteration with the switch on, and mdd_img_backward the full flat gradient."""
    eng = _engine("nfnet_tiny", "f32", 3, 0)
    inp = _inputs(eng, 3)
    image_syn, text_syn, lr, th0i, th0t = inp[:5]
    g = torch.Generator().manual_seed(7)
    vi = (torch.randn(eng.P_img, generator=g) * float(th0i.abs().mean())).to(eng.device)
    vt = (torch.randn(eng.P_txt, generator=g) * 0.05).to(eng.device)
    yb = torch.randn(N, eng.feature_dim, generator=g).to(eng.device)
    ybd = torch.randn(N, eng.feature_dim, generator=g).to(eng.device)

    def op_level():
        eng.img_forward(0, th0i, image_syn)
        gi = eng.img_backward(0, th0i, yb)
        eng.img_tangent_forward(0, th0i, vi)
        hi = eng.img_tangent_backward(0, th0i, vi, ybd)
        eng.txt_forward(0, th0t, text_syn)
        gt = eng.txt_backward(0, th0t, yb)
        eng.txt_tangent_forward(0, th0t, vt)
        ht = eng.txt_tangent_backward(0, th0t, vt, ybd)
        torch.cuda.synchronize()
        return dict(g_img=gi, Hv_img=hi, g_txt=gt, Hv_txt=ht)

    with skip_mode(1):
        before = op_level()
        _match(eng, inp, 3)
        after = op_level()
    table = {name: off for name, _, off in eng.param_table("img")}
    eng.close()
    for k in before:
        e = rel_err(after[k], before[k])
        report(f"unused_param_grads op-level {k}: after-vs-before an iteration {e:.2e}, norm {float(after[k].norm()):.3e}")
        assert float(before[k].norm()) > 0 and float(after[k].norm()) > 0, k
        assert e <= F32_TOL, (k, e)
    # the full flat gradient: no parameter tensor's slice has gone to zero (a norm-wise figure would hide a small one)
    offs = sorted(table.values()) + [after["g_img"].numel()]
    filled = 0
    for name, off in table.items():
        end = offs[offs.index(off) + 1]
        for k in ("g_img", "Hv_img"):
            was, now = float(before[k][off:end].abs().max()) > 0, float(after[k][off:end].abs().max()) > 0
            assert was == now, (k, name)
            filled += int(now)
    assert filled >= len(table), (filled, len(table))
