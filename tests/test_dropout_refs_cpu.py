"""The reference of the in-engine dropout mask (tests/dropout_refs.py) against published known-answer vectors and
against what a dropout mask must be, and the ABI-13 surface of the library (no GPU)."""
import ctypes as C
import os
import re

import numpy as np

import dropout_refs as R
from conftest import ROOT

# Random123's known-answer vectors for philox4x32-10: (counter, key) -> words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SEED = 0x0123456789abcdef


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        got = tuple(int(w) for w in R.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(g) for g in got])
    # vectorised over the counter as mask_words uses it
    c = np.array([k[0] for k in KAT], dtype=np.uint64).T
    k = np.array([k[1] for k in KAT], dtype=np.uint64).T
    got = np.stack(R.philox4x32_10(tuple(c), tuple(k)), 1)
    assert (got == np.array([k[2] for k in KAT], dtype=np.uint64)).all()


def test_counter_layout_of_the_mask():
    """Word column % 4 of the block (column // 4, sample, step, iteration) under key (seed low, seed high)."""
    n, d, step, it = 3, 10, 3, 7
    idx = np.array([8, 2, 5])
    w = R.mask_words(SEED, step, it, n, d, idx)
    for r in range(n):
        for c in range(d):
            blk = R.philox4x32_10((c // 4, int(idx[r]), step, it), (SEED & 0xffffffff, SEED >> 32))
            assert int(w[r, c]) == int(blk[c % 4])
    # sample id, not position: the rows of a subset are rows of the full mask
    full = R.mask(0.1, SEED, step, it, 9, d)
    assert (R.mask(0.1, SEED, step, it, n, d, idx) == full[idx]).all()
    assert (R.mask_words(SEED, step, it, n, d) == R.mask_words(SEED, step, it, n, d, np.arange(n))).all()


def test_mask_statistics_and_values():
    p, n, d = 0.1, 100, 2304
    m3 = R.mask(p, SEED, 3, 7, n, d)
    m4 = R.mask(p, SEED, 4, 7, n, d)
    assert m3.dtype == np.float32
    assert set(np.unique(m3).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))}
    keep = float((m3 != 0).mean())
    same = float((m3 == m4).mean())
    print("keep rate %.5f, equal entries between steps %.4f" % (keep, same))
    assert 0.895 <= keep <= 0.905          # 4 sigma = 0.0025 at 230400 draws
    assert 0.80 <= same <= 0.84            # independent masks: 0.9^2 + 0.1^2 = 0.82
    # another iteration and another seed give other masks as well
    assert 0.80 <= float((m3 == R.mask(p, SEED, 3, 8, n, d)).mean()) <= 0.84
    assert 0.80 <= float((m3 == R.mask(p, SEED + (1 << 32), 3, 7, n, d)).mean()) <= 0.84
    assert (R.mask(0.0, SEED, 3, 7, 5, 33) == np.float32(1.0)).all()


def _lib():
    from multimodal_dataset_distillation_amd import _lib, build_ext
    if not os.path.exists(_lib.LIB_PATH):
        build_ext.build(verbose=False)
    return _lib


def test_abi_13_exports_and_struct_size():
    L = _lib()
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.mdd_version() == 13
    for name in ("mdd_txt_forward_rng", "mdd_op_dropout_mask", "mdd_sizeof_iter_args"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.mdd_sizeof_iter_args() == C.sizeof(L.MddIterArgs)
    names = [f[0] for f in L.MddIterArgs._fields_]
    assert names[-3:] == ["drop_p", "drop_iteration", "drop_seed"]
    a = L.MddIterArgs()
    assert a.drop_p == 0.0 and a.drop_masks is None      # a zeroed struct asks for no dropout
    hdr = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    assert re.search(r"#define\s+MDD_ABI_VERSION\s+13\b", hdr) and "13 = +" in hdr


def test_argument_checks_need_no_gpu():
    """p outside [0, 1) is refused before anything touches the device."""
    L = _lib()
    lib = L.load()
    buf = (C.c_float * 8)()
    for p in (1.0, -0.1, float("nan"), 2.0):
        rc = lib.mdd_op_dropout_mask(p, SEED, 0, 0, 1, 8, None, C.cast(buf, C.c_void_p), None)
        assert rc != 0 and b"invalid argument" in lib.mdd_last_error()


def test_python_surface_has_the_keywords():
    import inspect
    from multimodal_dataset_distillation_amd import distill, buffer, engine, epoch, functional, networks, parallel
    assert "dropout" in inspect.signature(engine.UnrollEngine.txt_forward).parameters
    assert "dropout" in inspect.signature(engine.UnrollEngine.unrolled_match).parameters
    assert "dropout" in inspect.signature(functional.text_projection).parameters
    assert "dropout" in inspect.signature(parallel.sharded_unrolled_match).parameters
    assert "dropout" in inspect.signature(epoch.train_epoch).parameters
    assert inspect.signature(networks.ProjectionHead.__init__).parameters["rng"].default == "torch"
    assert callable(engine.dropout_mask)
    for mod in (distill, buffer):
        a, _ = mod.build_parser().parse_known_args([])
        assert a.dropout_rng == "torch"
        a, _ = mod.build_parser().parse_known_args(["--dropout_rng", "engine"])
        assert a.dropout_rng == "engine"
