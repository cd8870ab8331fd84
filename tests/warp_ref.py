"""float64 NumPy restatement of the time-warp operator (include/lipasr.h, lipasr_warp_apply), written from the formula and reading
the SAME fp32 tables as the library, so that only rounding separates it from the device and the host twins; the derived error
bounds of tests/test_warp_cpu.py and tests/test_warp_gpu.py; the clips and the model of their attack tests; and the float64
worst-of-grid driver and refinement over oracle.mfcc_ref and bounds_ref.forward that lipasr.attacks.TimeWarp is held against.
"""
from __future__ import annotations

import functools

import numpy as np

import bounds_ref as B
from oracle import mfcc_ref as M

Z, P = 16, 512
U = 2.0 ** -24
TRIPLES = [(0.0, 1.0, 1.0), (3.37, 1.0, 1.0), (-100.25, 1.07, 0.7), (12.5, 0.9, 1.4), (-7.0, 1.25, 1.0)]
NS = [1, 3, 37, 4099]


def nvs(n):
    return [0, 1, 2 * Z - 1, n]


@functools.lru_cache(maxsize=None)
def tables():
    import lipasr._native as N

    win, delta = N.warp_table_host()
    return win, delta


def table_formula():
    """win in float64, as the header states it."""
    i = np.arange(Z * P + 1, dtype=np.float64)
    w = np.sinc(i / P) * np.i0(8.6 * np.sqrt(np.maximum(0.0, 1.0 - (i / (Z * P)) ** 2))) / np.i0(8.6)
    w[P::P] = 0.0
    w[0] = 1.0
    return w


def warp_row(x, nv, shift, rate, gain):
    """One row in float64 -> dict(out, acc, dxu, absw, absd), each [n]: x float64 [n], nv the clamped length."""
    win, delta = (t.astype(np.float64) for t in tables())
    n = len(x)
    res = {k: np.zeros(n) for k in ("out", "acc", "dxu", "absw", "absd")}
    shift, rate, gain = float(shift), float(rate), float(gain)
    if not (np.isfinite(shift) and np.isfinite(gain) and 0.5 <= rate <= 2.0):
        res["out"][:nv] = np.nan
        res["acc"][:nv] = np.nan
        res["dxu"][:nv] = np.nan
        return res
    if nv == 0:
        return res
    t = np.arange(nv, dtype=np.float64)
    c = (nv - 1) / 2.0
    u = (c + rate * (t - c)) - shift
    u0 = np.floor(u)
    f = u - u0
    n0 = np.clip(u0, -(Z + 2), nv + Z + 1).astype(np.int64)
    acc, dxu, absw, absd = (np.zeros(nv) for _ in range(4))
    for wing in range(2):
        idx = (f if wing == 0 else 1.0 - f) * P
        j0 = idx.astype(np.int64)
        eta = (idx - j0).astype(np.float32).astype(np.float64)
        for i in range(Z):
            pos = n0 - i if wing == 0 else n0 + 1 + i
            j = j0 + i * P
            ok = (pos >= 0) & (pos < nv) & (j <= Z * P)
            jj, pp = np.minimum(j, Z * P), np.clip(pos, 0, nv - 1)
            xv = np.where(ok, x[pp], 0.0)
            w = win[jj] + eta * delta[jj]
            s = delta[jj] * (P if wing == 0 else -P)
            acc += w * xv
            dxu += s * xv
            absw += np.abs(w * xv)
            absd += np.abs(s * xv)
    res["acc"][:nv], res["dxu"][:nv], res["absw"][:nv], res["absd"][:nv] = acc, dxu, absw, absd
    res["out"][:nv] = gain * acc
    return res


def clamp_nv(n_valid, b, n):
    return n if n_valid is None else int(min(max(int(n_valid[b]), 0), n))


def warp_apply(x, params, K, n_valid=None, parts=False):
    """x [B, n], params [B * K, 3] -> out float64 [B * K, n]; parts=True: (out, [per-row dicts of warp_row])."""
    x = np.asarray(x, np.float64)
    params = np.asarray(params, np.float64)
    b, n = x.shape
    rows = [warp_row(x[r // K], clamp_nv(n_valid, r // K, n), *params[r]) for r in range(b * K)]
    out = np.stack([r["out"] for r in rows]) if rows else np.zeros((0, n))
    return (out, rows) if parts else out


def spacing32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def out_bound(row, gain):
    """|out32 - out64| <= (2 Z + 4) 2^-24 |gain| sum_k |w_k x_k| + spacing32(|out64|): a chain of 2 Z fused steps, the weight's own
    fma and the final product."""
    return (2 * Z + 4) * U * abs(gain) * row["absw"] + spacing32(row["out"])


def param_vjp(x, g, params, K, n_valid=None):
    """(gp float64 [B * K, 3], its bound [B * K, 3]): the three sums in float64, and what the fp32 chains under them may cost."""
    x, g, params = np.asarray(x, np.float64), np.asarray(g, np.float64), np.asarray(params, np.float64)
    b, n = x.shape
    gp, bound = np.zeros((b * K, 3)), np.zeros((b * K, 3))
    for r in range(b * K):
        nv = clamp_nv(n_valid, r // K, n)
        shift, rate, gain = params[r]
        row = warp_row(x[r // K], nv, shift, rate, gain)
        if np.isnan(row["out"][:nv]).any() or not (np.isfinite(shift) and np.isfinite(gain) and 0.5 <= rate <= 2.0):
            gp[r] = np.nan
            continue
        tc = np.arange(n, dtype=np.float64) - (nv - 1) / 2.0
        live = np.arange(n) < nv
        gg = np.where(live, g[r], 0.0)
        terms = np.stack([gg * gain * -row["dxu"], gg * gain * row["dxu"] * tc, gg * row["acc"]])
        gp[r] = terms.sum(axis=1)
        ed = (2 * Z + 4) * U * row["absd"] + spacing32(row["dxu"])
        ea = (2 * Z + 4) * U * row["absw"] + spacing32(row["acc"])
        bound[r] = [np.sum(np.abs(gg * gain) * ed), np.sum(np.abs(gg * gain) * ed * np.abs(tc)), np.sum(np.abs(gg) * ea)]
        bound[r] += 1e-12 * np.abs(terms).sum(axis=1)
    return gp, bound


def grid_case(n, nv, K, clips=3, seed=0):
    """(x float32 [clips, n], n_valid int32 [clips], params float32 [clips * K, 3], g float32 [clips * K, n]) of the twin and device
    tests: the first clip has the stated length, the others n and about half of it; the triples cycle through TRIPLES."""
    rng = np.random.default_rng(1000 * n + 10 * nv + K + seed)
    x = rng.standard_normal((clips, n)).astype(np.float32)
    n_valid = np.array([nv, n, nv // 2 + 1][:clips], dtype=np.int32)
    params = np.array([TRIPLES[(r + nv) % len(TRIPLES)] for r in range(clips * K)], dtype=np.float32)
    g = rng.standard_normal((clips * K, n)).astype(np.float32)
    return x, n_valid, params, g


# ----------------------------------------------------------------------------------------------------- the attack's test bed
SR16, N_SAMP, UTT = 16000, 4000, 8          # the extractor of the device tests: 16 kHz rows of 4 000 samples, 8 frames kept
N_Y = int(np.ceil(N_SAMP * 22050.0 / SR16))  # their 22 050 Hz rows: 5 513 positions
WIDTHS = [20 * UTT, 32, 5]
SEED = 1  # chosen so that test_warp_cpu.py::test_float64_drivers_are_not_vacuous holds (seeds 0 and 2 flip no label here)
RAMP = 32


def positions(lengths):
    """ceil(n * 22050 / sr_in) in float64, as WaveformClassifier.clip_positions counts."""
    return np.ceil(np.asarray(lengths, np.float64) * (22050.0 / SR16)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def clips(count=24, seed=SEED):
    """(x float32 [count, N_Y] at 22 050 Hz, lengths int32 [count] in samples at 16 kHz): harmonic bursts that fill their clips
    (ramps of RAMP positions at either end), zero beyond each clip's positions -- so that a delay moves silence in at one end."""
    rng = np.random.default_rng(100 + seed)
    # multiples of 320 samples, so that n * 22050 / 16000 is whole: where it is not, the extractor reads the clip's last position as
    # the zero that librosa's fix_length appends, whatever a warp has moved there
    lengths = (320 * rng.integers(7, 13, count)).astype(np.int32)
    x = np.zeros((count, N_Y), dtype=np.float32)
    for b, nv in enumerate(positions(lengths)):
        t = np.arange(nv) / 22050.0
        f0 = rng.uniform(110.0, 330.0)
        amps = rng.uniform(0.2, 1.0, 6) / np.arange(1, 7)
        s = sum(a * np.sin(2 * np.pi * f0 * (h + 1) * t + rng.uniform(0, 2 * np.pi)) for h, a in enumerate(amps))
        env = np.ones(nv)
        ramp = np.hanning(2 * RAMP)
        env[:RAMP], env[nv - RAMP:] = ramp[:RAMP], ramp[RAMP:]
        x[b, :nv] = (0.3 * s * env / np.abs(s).max()).astype(np.float32)
    return x, lengths


@functools.lru_cache(maxsize=None)
def model(seed=SEED):
    return B.make_model(WIDTHS, seed, signed=True)


def features(row, nv):
    """float64 features [20 * UTT] of the first nv positions of a 22 050 Hz row."""
    return M.fix_frames(M.mfcc_22k(np.asarray(row[:nv], np.float64), dtype=np.float64), UTT).flatten()


def logits(m, row, nv):
    return B.forward(m, features(row, nv))


def margin(z, y, targeted=False):
    """z_y - max_{k != y} z_k; targeted: its negative."""
    v = z[y] - np.max(np.delete(z, y))
    return -v if targeted else v


def margin_at(m, x, nv, triple, y, targeted=False):
    return margin(logits(m, warp_row(np.asarray(x, np.float64), nv, *triple)["out"], nv), y, targeted)


def own_labels(m, x, lengths):
    return np.array([int(np.argmax(logits(m, x[b], nv))) for b, nv in enumerate(positions(lengths))])


def worst_of_grid(m, x, lengths, grid, y, targeted=False):
    """(pick [B], margins [B, K], logits [B, K, C]) in float64: every clip under every triple of ``grid`` (float32 values, as the
    kernel reads them); the pick is the smallest margin, ties to the lowest index."""
    grid = np.asarray(grid, np.float32).astype(np.float64)
    pos = positions(lengths)
    zs = np.array([[logits(m, warp_row(x[b].astype(np.float64), int(pos[b]), *tr)["out"], int(pos[b])) for tr in grid]
                   for b in range(len(x))])
    ms = np.array([[margin(zs[b, j], y[b], targeted) for j in range(len(grid))] for b in range(len(x))])
    return ms.argmin(axis=1), ms, zs


def refine(m, x, nv, triple, y, lo, hi, step, steps, h=(1e-3, 1e-6, 1e-4), targeted=False):
    """The float64 refinement: projected sign steps on one clip's triple, the slope of the margin from central differences over the
    three parameters (no MFCC backward pass), a step kept only if the margin fell, halved otherwise."""
    p = np.array(triple, np.float64)
    step = np.array(step, np.float64)
    best = margin_at(m, x, nv, p, y, targeted)
    for _ in range(steps):
        d = np.zeros(3)
        for q in range(3):
            if step[q] == 0.0:
                continue
            e = np.zeros(3)
            e[q] = h[q]
            d[q] = margin_at(m, x, nv, p + e, y, targeted) - margin_at(m, x, nv, p - e, y, targeted)
        cand = np.clip(p - step * np.sign(d), lo, hi)
        got = margin_at(m, x, nv, cand, y, targeted)
        if got < best:
            p, best = cand, got
        else:
            step = 0.5 * step
    return p, best
