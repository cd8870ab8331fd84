"""Philox4x32-10 (Salmon et al. 2011), restated once for every oracle of the attack kernels, and the n_valid clamp they share.
TEST INFRASTRUCTURE for tests/*_ref.py: nothing here is used by the library.

    philox        one block on Python integers only
    philox_np     blocks on uint64 arrays (pinned against ``philox`` by test_hsj_cpu, against Random123's known answers by
                  test_dropout_quads_gpu)
    nv            n_valid[b] clamped to [0, n]; n without lengths
"""
from __future__ import annotations

import numpy as np

MASK = 0xFFFFFFFF
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(MASK)


def philox(seed, ctr_lo, hi0, hi1):
    """One block: key ``seed`` (64 bits), counter (ctr_lo low word, ctr_lo high word, hi0, hi1) -> four 32-bit words."""
    c = [ctr_lo & MASK, (ctr_lo >> 32) & MASK, hi0 & MASK, hi1 & MASK]
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def philox_np(seed, lo, hi, hi0, hi1):
    """Blocks with key ``seed`` and counters (lo, hi, hi0, hi1), each a 32-bit value or array -> uint64 array [4, ...]."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(lo, hi, hi0, hi1)]
    k0, k1 = np.uint64(seed & MASK), np.uint64((seed >> 32) & MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 bits: no overflow in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return np.stack(c)


def nv(n_valid, b, n):
    return n if n_valid is None else min(max(int(n_valid[b]), 0), n)
