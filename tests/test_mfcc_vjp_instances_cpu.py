"""CPU companion of test_mfcc_vjp_instances_gpu.py: the per-stage references of the MFCC backward pass (tests/mfcc_vjp_stage_ref.py) are
right, and their bounds are decisive.

  * the stages compose to the oracle: stage 1, then stages 2+3, then stage 4, all in float64, equal mfcc_grad_ref.vjp (autograd through the
    float64 forward) to 1e-9 relative on the guard-clear parity clips, for 2048/512 at 16 kHz and for 441/220;
  * every wrong restatement exceeds the bound of the GPU case it belongs to, at F_MAX = 32, the largest factor a kernel may be given
    (so at whatever factor is chosen): stage 1 per element against F 2^-24 A, stages 2+3 in the metric of mfcc_grad_ref.errs against
    F x the float32 restatement's error, stage 4 per element against (nt + 1) 2^-24 sum |h| |g_y|;
  * the inputs meet their conditions, asserted by count: ties in different frames, elements on, above and below the floor, a maximum
    in a frame >= L.

One restatement of the issue cannot be seen by any test, by construction: "bins 0 and 1024 doubled".  The mel bank has fmin = 0 and fmax =
sr / 2, so its weights at bin 0 and at bin N/2 are exactly 0 for every filter and every n_fft: GP = W^T Gmel is exactly 0 there, and so is
Z = 2 GP X, doubled or not.  The test asserts the zero columns and that the restatement changes no bit, and asks the bound of the nearest
visible mistake instead: bins 1 and N/2 - 1 doubled ('edge1').

Two exemptions, by reasoning.  A clip of n_y = 2 samples [a, b] is reflected into the period-2 signal a b a b ...: the fold maps every
even padded position to sample 0 and every odd one to sample 1, so a symmetric and a periodic window, whose samples differ, are told
apart, but the 'fold' restatement (defined for the single reflection of a clip longer than the padding) is not asked of clips of
n_y <= n_fft.  Stage 4's 't0' and tap restatements are asked of the resampling rates only: the identity copies.
"""
import numpy as np
import pytest
import torch

import mfcc_grad_ref as G
import mfcc_stage_ref as S
import mfcc_vjp_stage_ref as V
from oracle import mfcc_ref as M


# ---------------------------------------------------------------------------------------------- the stages compose to the oracle
def _compose(x, g_feat, L, scale, sr, n_fft, hop):
    """stage 1 o stages 2+3 o stage 4 in float64 from the float64 forward's own tile"""
    xt = torch.as_tensor(np.asarray(x, np.float64))
    with torch.no_grad():
        y = (xt if sr == V.SR else G.resample(xt, sr)).numpy()
        db = G.db_22k(torch.as_tensor(y), n_fft=n_fft, hop=hop).numpy()
    T = db.shape[0]
    gmel, _ = V.stage1(db, db.max(axis=1), g_feat, L, T, scale, cmp=np.float64)
    gy, _ = V.stage23(y, gmel, n_fft, hop)
    if sr == V.SR:
        return gy
    return V.resample_vjp(gy, len(x), sr, V.oracle_tables(sr, rounded=False))[0]


@pytest.mark.parametrize("n_fft,hop,sr", [(2048, 512, 16000), (441, 220, 22050)])
def test_stages_compose_to_the_autograd_oracle(n_fft, hop, sr):
    L = 44
    if n_fft == 2048:
        clips = G.parity_clips(12000)  # 33 frames < L; the 20000-sample clips (54 frames > L) below
        clips2 = G.parity_clips(20000)[:2]
        sets = [(c, "input") for c in clips] + [(c, "input") for c in clips2]
    else:
        sets = [(c, "22k") for c in G.short_parity_clips(441, 220, 22050)]  # 101 frames > L
    g_feat, scale = V.case_cotangent(L)
    for i, (x, domain) in enumerate(sets):
        y22 = x if domain == "22k" else M.librosa_load_resample(x, sr, dtype=np.float64)
        dist, gap, _ = G.guard_margins(y22, n_fft, hop)
        assert dist > 1e-6 and gap > 1e-6, (i, dist, gap)  # the parity clips keep clear of the floor and of ties
        want = G.vjp(x, g_feat, sr, L, scale, domain=domain, n_fft=n_fft, hop=hop)
        got = _compose(x, g_feat, L, scale, sr, n_fft, hop)
        e_inf, e_2 = G.errs(got, want)
        assert e_inf < 1e-9 and e_2 < 1e-9, (n_fft, i, e_inf, e_2)


# ---------------------------------------------------------------------------------------------- stage 1
def _loud_last_tile():
    return V.tile_from_clip(S.loud_last_clip(2205))


def test_stage1_inputs_meet_their_conditions():
    db, fmax = V.tie_tile()
    t, m = np.nonzero(db == db.max())
    assert len(t) >= 2 and len(set(t.tolist())) >= 2 and (fmax == db.max(axis=1)).all()
    assert (db <= db.max() - np.float32(80.0)).sum() >= 1  # a floored sum that the tie decides the place of
    db, fmax = V.floor_tile()
    thr = np.float32(db.max() - np.float32(80.0))
    assert (db == db.max()).sum() == 1
    assert (db == thr).sum() >= 5 and (db > thr).sum() >= 100 and ((db < thr) & (db > np.float32(-100.0))).sum() >= 20
    assert (db == np.nextafter(thr, np.float32(0.0))).sum() >= 5 and (db == np.nextafter(thr, np.float32(-200.0))).sum() >= 5
    assert (db == np.float32(-100.0)).sum() >= 4
    db, fmax = _loud_last_tile()
    L = 4
    assert db.shape[0] == 5 and int(fmax.argmax()) >= L and fmax.max() - fmax[:L].max() > 1.0
    assert (db <= db.max() - np.float32(80.0)).sum() >= 100
    db, fmax = V.last_element_tile()
    assert np.flatnonzero(db.ravel() == db.max()).tolist() == [db.size - 1]


@pytest.mark.parametrize("wrong,tile,L", [("last", "tie", 44), ("last", "tie", 4), ("ge", "floor", 44), ("drop", "floor", 44), ("drop", "tie", 4),
                                          ("firstL", "loud-last", 4), ("mul", "floor", 44), ("mul", "loud-last", 4)])
def test_stage1_bound_is_decisive(wrong, tile, L):
    db, fmax = {"tie": V.tie_tile, "floor": V.floor_tile, "loud-last": _loud_last_tile}[tile]()
    g_feat, scale = V.case_cotangent(L)
    val, A = V.stage1(db, fmax, g_feat, L, 5, scale)
    bad, _ = V.stage1(db, fmax, g_feat, L, 5, scale, wrong=wrong)
    assert np.isfinite(val).all() and np.isfinite(A).all() and (np.abs(val) <= A * (1 + 1e-12)).all()
    assert (A[db > np.float32(-100.0)][:128 * min(5, L)] >= 0).all()
    excess = np.abs(bad - val) - V.F_MAX * V.U * A
    print(f"{wrong} on the {tile} tile, L {L}: worst |wrong - right| / (2^-24 A) = {(np.abs(bad - val) / np.where(A > 0, V.U * A, 1.0)).max():.3e}")
    assert excess.max() > 0.0, (wrong, tile, L)
    assert V.F1 <= V.F_MAX


def test_stage1_exact_zeros():
    g_feat, scale = V.case_cotangent(3)
    val, A = V.stage1(*V.dead_tile(), g_feat, 3, 5, scale)
    assert not val.any() and not A.any()
    db, fmax = V.tie_tile()
    val, A = V.stage1(db, fmax, g_feat, 3, 5, scale)
    assert not val[3:].any() and val[3, 7] == 0.0 and val[1, 40] != 0.0  # frames >= L: nothing; the later maxima get no floored sum


# ---------------------------------------------------------------------------------------------- stages 2 + 3
S23_SHAPES = [(2048, 512, n) for n in (2, 56, 552, 2048, 2050, 4135, 9647)] + [(f, h, n) for f, h, n in V.SHORT_SHAPES]


@pytest.mark.parametrize("n_fft,hop,n_y", S23_SHAPES)
def test_stage23_bound_is_decisive(n_fft, hop, n_y):
    y = V.case_clip(n_y)
    T = 1 + (n_y + 2 * (n_fft // 2) - n_fft) // hop
    assert T == 1 + n_y // hop
    gmel = V.random_gmel(T)
    ref, reached = V.stage23(y, gmel, n_fft, hop)
    yard = V.errs(V.stage23(y, gmel, n_fft, hop, dtype=torch.float32)[0], ref)
    assert reached.all() and 0.0 < yard[0] < 1e-5 and 0.0 < yard[1] < 1e-5, yard
    W = M.mel_filterbank(n_fft=n_fft)
    assert not W[:, 0].any() and (n_fft % 2 or not W[:, -1].any()) and W[:, 1].any()  # see the module docstring
    assert np.array_equal(V.stage23(y, gmel, n_fft, hop, wrong="edge2")[0], ref)
    for wrong in ("edge1", "late", "hann", "fold"):
        if wrong == "fold" and n_y <= n_fft:
            continue  # see the module docstring
        bad = V.errs(V.stage23(y, gmel, n_fft, hop, wrong=wrong)[0], ref)
        print(f"{n_fft}/{hop} n_y {n_y}: float32 yardstick {yard[0]:.2e} {yard[1]:.2e}; wrong '{wrong}' {bad[0]:.2e} {bad[1]:.2e}")
        assert bad[0] > V.F_MAX * yard[0] and bad[1] > V.F_MAX * yard[1], (wrong, bad, yard)
    assert max(V.F2.values()) <= V.F_MAX


def test_stage23_zero_cotangent_frames_reach_nothing():
    """n_y = 4135, 9 frames, frames >= 4 zero: the samples past frame 3's window are exactly 0 in the reference"""
    y = V.case_clip(4135)
    ref, reached = V.stage23(y, V.random_gmel(9, range(4)))
    assert reached[:3 * 512 + 1024].all() and not reached[3 * 512 + 1024:].any()
    assert not ref[~reached].any() and np.count_nonzero(ref[reached]) > 2000


# ---------------------------------------------------------------------------------------------- stage 4
@pytest.mark.parametrize("sr,n", [(16000, 1487), (8000, 1500), (16010, 3300)])
def test_stage4_bound_is_decisive(sr, n):
    tab = V.oracle_tables(sr)
    nt = V.adjoint_taps(tab)
    assert 128 * tab[1] // tab[2] <= nt <= 128 * tab[1] // tab[2] + 3, nt  # ~ taps up / down
    n_vy, n_y, _ = V.clip_lengths(n, sr)
    gy = np.random.default_rng(sr + n).standard_normal(n_y).astype(np.float32)
    ref, mag = V.resample_vjp(gy, n, sr, tab)
    bound = (nt + 1) * V.U * mag
    # the reference is the adjoint of the oracle's forward: <R x, g_y> = <x, R^T g_y>
    x = np.random.default_rng(1).standard_normal(n)
    Rx = G.resample(torch.as_tensor(x), sr).numpy()
    assert abs(Rx[:n_y] @ gy.astype(np.float64) - x @ V.resample_vjp(gy, n, sr, V.oracle_tables(sr, rounded=False))[0]) < 1e-9 * np.abs(Rx).sum()
    # a frame of reference one sample off belongs to the dense case and its a-priori bound ...
    bad, _ = V.resample_vjp(gy, n, sr, tab, wrong="t0")
    print(f"{sr} Hz: 't0' worst |wrong - right| / bound = {(np.abs(bad - ref) / bound).max():.3e}")
    assert (np.abs(bad - ref) > bound).any()
    # ... a dropped end tap to the comb case, whose bound is zero: the end taps of the Kaiser window are ~1e-7 of the centre ones, far
    # inside the dense bound (printed), which is why the GPU suite pins every tap with unit impulses, bit for bit
    spacing = nt + 3
    rows = V.comb_rows(n_y, n_vy, spacing)[:3]
    for wrong in ("first", "last"):
        dense, _ = V.resample_vjp(gy, n, sr, tab, wrong=wrong)
        print(f"{sr} Hz: '{wrong}' on the dense case: worst |wrong - right| / bound = {(np.abs(dense - ref) / bound).max():.3e} (not decisive)")
        differ = sum(int(np.count_nonzero(V.resample_vjp(r, n, sr, tab, wrong=wrong)[0] != V.resample_vjp(r, n, sr, tab)[0])) for r in rows)
        assert differ >= 3, (wrong, differ)
    if n_vy < n_y:  # the appended zero sample gives nothing
        g2 = gy.copy()
        g2[n_vy] += 1.0
        assert np.array_equal(V.resample_vjp(g2, n, sr, tab)[0], ref)


def test_stage4_comb_rows_see_one_tap_each():
    tab = V.oracle_tables(16000)
    nt = V.adjoint_taps(tab)
    n = 1487
    n_vy, n_y, _ = V.clip_lengths(n, 16000)
    spacing = nt + 3
    rows = V.comb_rows(n_y, n_vy, spacing)
    assert rows.shape == (spacing, n_y) and rows[:, :n_vy].sum(axis=0).tolist() == [1.0] * n_vy and (rows[:, n_vy] == 1.0).all()
    taps = set(np.unique(tab[0]).tolist())
    seen = set()
    for s in (0, 1, spacing - 1):
        g, mag = V.resample_vjp(rows[s], n, 16000, tab)
        assert np.array_equal(np.abs(g), mag)  # at most one impulse per g_x sample: nothing is summed
        assert set(np.unique(g).tolist()) <= taps | {0.0}
        seen |= set(np.unique(g).tolist())
    assert len(seen) > 1000
