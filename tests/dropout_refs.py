"""numpy restatement of the dropout mask the engine draws inside its text-head kernels (include/mdd_hip.h
mdd_txt_forward_rng; csrc/philox.h).  Integer arithmetic in uint64 with explicit 32-bit wrap, written from the
definition alone:

  generator  Philox4x32-10 (Salmon et al., SC'11): ten rounds of
                 (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
             with M0 = 0xD2511F53, M1 = 0xCD9E8D57 and the key bumped by (0x9E3779B9, 0xBB67AE85) between rounds
  key        (seed low 32 bits, seed high 32 bits)
  counter    (column // 4, sample, step, iteration); output word column % 4 belongs to `column`
  sample     (uint32) idx[row] when a row index vector is given, else row
  value      u = float32(word >> 8) * 2^-24; keep iff u >= float32(p); mask = keep ? float32(1) / (float32(1) - float32(p)) : 0
"""
import numpy as np

_U = np.uint64
M0, M1 = _U(0xD2511F53), _U(0xCD9E8D57)
W0, W1 = _U(0x9E3779B9), _U(0xBB67AE85)
LOW = _U(0xFFFFFFFF)
S32 = _U(32)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit values, key: 2.  Returns the 4 output words as uint64 arrays < 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LOW for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & LOW for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2          # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LOW, (p0 >> S32) ^ c3 ^ k1, p0 & LOW
        k0, k1 = (k0 + W0) & LOW, (k1 + W1) & LOW
    return c0, c1, c2, c3


def mask_words(seed, step, iteration, n, d, idx=None):
    """[n, d] uint64: the 32-bit word of every (row, column)."""
    seed = int(seed) & (2 ** 64 - 1)
    sample = np.arange(n, dtype=np.uint64) if idx is None else (np.asarray(idx).astype(np.int64).astype(np.uint64) & LOW)
    assert sample.shape == (n,)
    col = np.arange(d, dtype=np.uint64)
    c0 = np.broadcast_to((col // _U(4))[None, :], (n, d))
    c1 = np.broadcast_to(sample[:, None], (n, d))
    w = philox4x32_10((c0, c1, _U(int(step)), _U(int(iteration))), (_U(seed & 0xFFFFFFFF), _U(seed >> 32)))
    sel = np.broadcast_to((col % _U(4))[None, :], (n, d))
    return np.choose(sel.astype(np.int64), [np.broadcast_to(x, (n, d)) for x in w])


def keep_pattern(p, seed, step, iteration, n, d, idx=None):
    u = (mask_words(seed, step, iteration, n, d, idx) >> _U(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def mask(p, seed, step, iteration, n, d, idx=None):
    """[n, d] float32 mask: 0 or 1 / (1 - p)."""
    return np.where(keep_pattern(p, seed, step, iteration, n, d, idx), scale(p), np.float32(0.0)).astype(np.float32)
