"""CPU suite: the C-ABI library loads and exports every symbol include/lipasr.h declares, its host-side
tables equal the oracle's, argument validation works without a GPU, and the host logic of the package
(datasets, visit orders, shard bounds) behaves like the reference."""
import os
import re

import numpy as np
import pytest

import lipasr._native as N
from lipasr import keras as K
from lipasr.Constraints import simple_norm_constraint
from lipasr.parallel import shard_bounds
from oracle import mfcc_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "lipasr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lipasr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    syms = declared_symbols()
    assert len(syms) >= 40
    for s in syms:
        assert hasattr(N.lib, s), f"{s} declared in include/lipasr.h but not exported"
    assert set(N.PROTOTYPES) == set(syms), set(N.PROTOTYPES) ^ set(syms)
    assert N.lib.lipasr_version() >= 200


def test_k3_launch_counters_without_gpu():
    """lipasr_debug_k3_launches (version 630): host-side counters, readable without a GPU; -1 for an id that does not exist."""
    assert N.lib.lipasr_version() >= 630 and N.has("lipasr_debug_k3_launches")
    assert N.lib.lipasr_debug_k3_launches(0) >= 0
    assert N.lib.lipasr_debug_k3_launches(-1) == -1 and N.lib.lipasr_debug_k3_launches(1000) == -1
    known = [k for k in range(64) if N.lib.lipasr_debug_k3_launches(k) >= 0]
    assert known == list(range(len(known))) and len(known) == 13  # the ids documented in include/lipasr.h, without gaps


def test_k1_launch_counters_and_stage_hook_without_gpu():
    """lipasr_debug_k1_launches and lipasr_debug_mfcc_stage (version 640): both exported; the counters are host-side and readable
    without a GPU, -1 for an id that does not exist, and the known ids are exactly 0..17 as include/lipasr.h lists them; the copy
    hook refuses a null plan before it touches a device."""
    assert N.lib.lipasr_version() >= 640 and N.has("lipasr_debug_k1_launches") and N.has("lipasr_debug_mfcc_stage")
    assert hasattr(N.lib, "lipasr_debug_k1_launches") and hasattr(N.lib, "lipasr_debug_mfcc_stage")
    assert N.lib.lipasr_debug_k1_launches(0) >= 0
    assert N.lib.lipasr_debug_k1_launches(-1) == -1 and N.lib.lipasr_debug_k1_launches(18) == -1 and N.lib.lipasr_debug_k1_launches(1000) == -1
    known = [k for k in range(64) if N.lib.lipasr_debug_k1_launches(k) >= 0]
    assert known == list(range(18))
    assert N.lib.lipasr_debug_mfcc_stage(None, 0, 1, None, None) == N.EINVAL
    assert "null argument" in N.last_error()


def test_k1_backward_hooks_without_gpu():
    """lipasr_debug_k1_vjp_launches, lipasr_debug_mfcc_vjp_stage and lipasr_debug_mfcc_stage_put (version 690): exported; the counters
    are host-side, -1 for an id that does not exist, and the known ids are exactly 0..12 as include/lipasr.h lists them; the two copy
    hooks refuse a null plan before they touch a device."""
    names = ("lipasr_debug_k1_vjp_launches", "lipasr_debug_mfcc_vjp_stage", "lipasr_debug_mfcc_stage_put")
    assert N.lib.lipasr_version() >= 690 and all(N.has(n) and hasattr(N.lib, n) and N.SINCE[n] == 690 for n in names)
    assert N.lib.lipasr_debug_k1_vjp_launches(-1) == -1 and N.lib.lipasr_debug_k1_vjp_launches(13) == -1
    assert [k for k in range(64) if N.lib.lipasr_debug_k1_vjp_launches(k) >= 0] == list(range(13))
    for fn in (N.lib.lipasr_debug_mfcc_vjp_stage, N.lib.lipasr_debug_mfcc_stage_put):
        assert fn(None, 0, 1, None, None) == N.EINVAL
        assert "null argument" in N.last_error()


def test_k2_launch_counters_and_stage_hook_without_gpu():
    """lipasr_debug_k2_launches and lipasr_debug_mlp_stage (version 730): both exported and declared; the counters are host-side and
    readable without a GPU, -1 for an id that does not exist, and the known ids are exactly 0..8 as include/lipasr.h lists them; the
    copy hook refuses null arguments before it touches a device."""
    names = ("lipasr_debug_k2_launches", "lipasr_debug_mlp_stage")
    assert N.lib.lipasr_version() >= 730 and all(N.has(n) and hasattr(N.lib, n) and N.SINCE[n] == 730 and n in N.PROTOTYPES for n in names)
    assert all(n in declared_symbols() for n in names)
    assert N.lib.lipasr_debug_k2_launches(0) >= 0
    assert N.lib.lipasr_debug_k2_launches(-1) == -1 and N.lib.lipasr_debug_k2_launches(9) == -1 and N.lib.lipasr_debug_k2_launches(1000) == -1
    assert [k for k in range(64) if N.lib.lipasr_debug_k2_launches(k) >= 0] == list(range(9))
    assert N.lib.lipasr_debug_mlp_stage(None, 0, 0, 1, None, None) == N.EINVAL
    assert "null argument" in N.last_error()
    import ctypes

    dst = ctypes.c_float()
    assert N.lib.lipasr_debug_mlp_stage(None, 0, 0, 1, ctypes.byref(dst), None) == N.EINVAL  # a null plan with a destination
    assert "null argument" in N.last_error()


def test_error_convention_without_gpu():
    assert N.lib.lipasr_create(0, None) == N.EINVAL
    assert "out is null" in N.last_error()
    with pytest.raises(ValueError):
        N.check(N.lib.lipasr_destroy(None))
    assert N.lib.lipasr_debug_table(99, 16000, None, 0) == N.EINVAL
    assert N.lib.lipasr_mlp_destroy(None) == N.EINVAL


def test_tables_equal_oracle():
    np.testing.assert_array_equal(N.debug_table(0), M.hann_periodic().astype(np.float32))
    np.testing.assert_allclose(N.debug_table(1).reshape(20, 128), M.dct_matrix(), atol=1e-7)
    np.testing.assert_array_equal(N.debug_table(2).reshape(128, 1025), M.mel_filterbank())
    # the two-filters-per-bin form the STFT kernel applies expands to the same dense bank, bit for bit
    np.testing.assert_array_equal(N.debug_table(8).reshape(128, 1025), M.mel_filterbank())


def test_banded_resampler_tables():
    """The MFMA resampler's banded taps reproduce the oracle (NumPy emulation of the kernel's index math)."""
    for sr in (16000, 8000):
        up, down, taps, left = (int(v) for v in N.debug_table(4, sr))
        hb = N.debug_table(6, sr).reshape(-1, 152, 32).astype(np.float64)
        lo = N.debug_table(7, sr).astype(int)
        x = np.random.default_rng(sr).standard_normal(sr // 2).astype(np.float32)
        ref = M.resample_kaiser_best(x, sr, 22050)
        nq = (len(ref) + up - 1) // up
        y = np.zeros(nq * up + 64)
        for q0 in range(0, nq, 2):
            xs = np.zeros(801)
            for t in range(2 * down + 127):
                n = down * q0 - (left - 1) + t
                if 0 <= n < len(x):
                    xs[t] = x[n]
            for r in range(len(lo)):
                for ql in range(2):
                    if q0 + ql < nq:
                        out = xs[lo[r] + ql * down: lo[r] + ql * down + 152] @ hb[r]
                        n_ph = min(32, up - 32 * r)
                        y[(q0 + ql) * up + 32 * r: (q0 + ql) * up + 32 * r + n_ph] = out[:n_ph]
        np.testing.assert_allclose(y[:len(ref)], ref, atol=2e-6)


@pytest.mark.parametrize("sr_in,n", [(16000, 3000), (8000, 1500), (44100, 6000), (48000, 6000)])
def test_polyphase_table_reproduces_resampy(sr_in, n):
    up, down, taps, left = (int(v) for v in N.debug_table(4, sr_in))
    H = N.debug_table(3, sr_in).reshape(up, taps).astype(np.float64)
    off = N.debug_table(5, sr_in).astype(int)
    x = np.random.default_rng(sr_in).standard_normal(n).astype(np.float32)
    ref = M.resample_kaiser_best(x, sr_in, 22050)
    xp = np.concatenate([np.zeros(left - 1), x.astype(np.float64), np.zeros(taps + down)])
    y = np.array([H[t % up] @ xp[down * (t // up) + off[t % up]: down * (t // up) + off[t % up] + taps] for t in range(len(ref))])
    keep = np.ones(len(ref), dtype=bool)
    if sr_in > 22050:
        # Down-sampling: resampy truncates the table step to an integer (int(scale*512)), so at outputs whose
        # time is an exact integer the result depends on whether the float time register lands just below or
        # on the integer (accumulate vs multiply differ by ~6e-4 there).  The table uses the exact rational
        # time; those phase-0 outputs are compared with the 'multiply' register instead.  The reference's
        # own corpus is 16 kHz (up-sampling, step exactly 512), where no such dependence exists.
        alt = M.resample_kaiser_best(x, sr_in, 22050, time_mode="multiply")
        keep = np.abs(ref - alt) < 1e-6
        assert keep.mean() > 0.99 and np.all(np.arange(len(ref))[~keep] % up == 0)
        np.testing.assert_allclose(y[~keep], alt[~keep], atol=3e-6 * max(1.0, np.abs(ref).max()))
    np.testing.assert_allclose(y[keep], ref[keep], atol=3e-6 * max(1.0, np.abs(ref).max()))


def test_dataset_shuffle_batch_structure():
    x = np.arange(2000)[:, None].astype(np.float32)
    ds = K.Dataset.from_tensor_slices((x, x)).shuffle(880, reshuffle_each_iteration=False, seed=3).batch(512)
    assert len(ds) == 4
    order = ds.order
    assert sorted(order) == list(range(2000)) and all(order[i] < i + 880 for i in range(2000))
    with pytest.raises(NotImplementedError):
        K.Dataset.from_tensor_slices((x, x)).shuffle(10, reshuffle_each_iteration=True)


def test_to_categorical_and_names():
    y = K.to_categorical([0, 2, 1], 3)
    np.testing.assert_array_equal(y, np.eye(3, dtype=np.float32)[[0, 2, 1]])
    K.reset_layer_names()
    names = [K.Dense(4, activation="relu").name for _ in range(3)] + [K.BatchNormalization().name, K.Dropout(0.1).name]
    assert names == ["dense", "dense_1", "dense_2", "batch_normalization", "dropout"]
    assert all("dense" in n for n in names[:3]) and "batch" in names[3]
    with pytest.raises(NotImplementedError):
        K.Dense(4, activation="tanh")


def test_visit_order_follows_reference_loops():
    c = simple_norm_constraint(0.1, [])
    assert c._visit_order(6) == [0, 1, 2, 3, 4, 5]
    c = simple_norm_constraint(0.1, [0, 2, 2, 5])
    assert c._visit_order(6) == [5, 2, 2, 0]  # Constraints.py:181-189: reversed layers, once per occurrence


def test_shard_bounds_cover_batch():
    for n, w in [(8192, 8), (182, 8), (7, 2), (512, 1)]:
        parts = [shard_bounds(n, r, w) for r in range(w)]
        assert parts[0][0] == 0 and parts[-1][1] == n
        assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
        assert max(b - a for a, b in parts) - min(b - a for a, b in parts) <= 1


def test_no_cpu_fallback_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.get_handle()
