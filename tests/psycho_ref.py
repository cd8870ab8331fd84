"""NumPy restatement of the psychoacoustic masker and of the imperceptible attack's loss (include/lipasr.h, "psychoacoustic
masking threshold"): tables, PSD, maskers with the greedy merge, the linear threshold, the hinge loss with its gradient to the
samples, and one attack step.  ``dtype=np.float64`` is the oracle; ``dtype=np.float32`` evaluates the same expressions in single
precision (SciPy's pocketfft keeps float32) and is the yardstick the device errors are held against.

The masker functions also return a ``margin``: the smallest |difference| in dB among the discrete comparisons they made (level
against the absolute threshold of hearing, level against level in the merge).  A frame with a tiny margin can legitimately
come out differently in float32, so the device tests leave those frames out (and cap how many there may be)."""
import numpy as np
from scipy import fft as sfft

N, HOP, K = 2048, 512, 1025
SIZES = (2048, 2560, 3072, 6244, 22050)   # one frame, a pair, an odd tail, 9 frames + 100 loose samples, 40 frames
RATES = (22050, 16000)
MARGIN_DB = 1e-4          # frames whose decisions are closer than this are not compared
MAX_LEFT_OUT = 0.02       # ... and at most this share of the frames may be


def n_frames(n):
    if n < N:
        raise ValueError(f"n={n} < {N}: not one whole window")
    return 1 + (n - N) // HOP


def tables(sr):
    """f, bark, ATH (dB, -inf outside 20 Hz .. 20 kHz), shift: float64 [1025]."""
    f = np.arange(K, dtype=np.float64) * sr / N
    bark = 13.0 * np.arctan(0.00076 * f) + 3.5 * np.arctan((f / 7500.0) ** 2)
    q = f / 1000.0
    ath = np.full(K, -np.inf)
    ok = (f >= 20.0) & (f <= 20000.0)
    ath[ok] = 3.64 * q[ok] ** -0.8 - 6.5 * np.exp(-0.6 * (q[ok] - 3.3) ** 2) + 0.001 * q[ok] ** 4 - 12.0
    return f, bark, ath, -6.025 - 0.275 * bark


def hann(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(dtype)


def stft(x, dtype=np.float64):
    """[n] -> X [T, 1025] of the Hann-windowed frames x[512 t : 512 t + 2048], computed in ``dtype``."""
    x = np.asarray(x, dtype=dtype)
    t = n_frames(len(x))
    idx = HOP * np.arange(t)[:, None] + np.arange(N)[None, :]
    return sfft.rfft(x[idx] * hann(dtype), axis=1)


def psd(x, dtype=np.float64):
    """-> (psd [T, 1025] in dB, psd_max)."""
    mag = np.abs(stft(x, dtype)).astype(dtype)
    with np.errstate(divide="ignore"):
        p = np.maximum(dtype(-200.0), dtype(20.0) * np.log10(dtype(np.sqrt(8.0 / 3.0)) * mag / dtype(N)))
    mx = p.max()
    return (dtype(96.0) - mx + p).astype(dtype), dtype(mx)


def merge(levels, bins, bark, bark_by="bin"):
    """The greedy merge on ascending lists -> (keep mask, margin)."""
    if bark_by not in ("bin", "position"):
        raise ValueError(bark_by)
    keep = np.ones(len(levels), dtype=bool)
    margin = np.inf
    at = (lambda i: bark[i]) if bark_by == "position" else (lambda i: bark[bins[i]])
    ip = 0
    for i in range(1, len(levels)):
        if at(i) - at(ip) < 0.5:
            margin = min(margin, abs(float(levels[ip]) - float(levels[i])))
            if levels[ip] < levels[i]:
                keep[ip] = False
                ip = ip + 1
            else:
                keep[i] = False
        else:
            ip = i
    return keep, margin


def maskers(v, tabs, bark_by="bin", dtype=np.float64):
    """One frame v [1025] (dB) -> (bins, levels, margin) of the surviving maskers."""
    _, bark, ath, _ = tabs
    v = np.asarray(v, dtype=dtype)
    k = np.arange(1, K - 1)
    cand = k[(v[k] > v[k - 1]) & (v[k] > v[k + 1])]
    ten = dtype(10.0)
    level = (ten * np.log10(ten ** (v[cand - 1] / ten) + ten ** (v[cand] / ten) + ten ** (v[cand + 1] / ten))).astype(dtype)
    a = ath[cand]
    fin = np.isfinite(a)
    margin = float(np.abs(level[fin].astype(np.float64) - a[fin]).min()) if fin.any() else np.inf
    ok = level > a
    cand, level = cand[ok], level[ok]
    keep, m2 = merge(level, cand, bark, bark_by)
    return cand[keep], level[keep], min(margin, m2)


def threshold(p, sr, bark_by="bin", dtype=np.float64):
    """psd [T, 1025] (dB, any PSD) -> (theta [T, 1025] linear, n_maskers [T], margin [T])."""
    tabs = tables(sr)
    _, bark, ath, shift = tabs
    with np.errstate(over="ignore"):
        ath_lin = np.where(np.isinf(ath), 0.0, 10.0 ** (ath / 10.0)).astype(dtype)
    barkd, shiftd, ten = bark.astype(dtype), shift.astype(dtype), dtype(10.0)
    theta = np.empty((len(p), K), dtype=dtype)
    count, margin = np.zeros(len(p), dtype=np.int64), np.zeros(len(p))
    for t, v in enumerate(p):
        bins, level, margin[t] = maskers(v, tabs, bark_by, dtype)
        count[t] = len(bins)
        dz = barkd[:, None] - barkd[bins][None, :]
        slope = dtype(-27.0) + dtype(0.37) * np.maximum(level - dtype(40.0), dtype(0.0))
        sf = np.where(dz <= 0, dtype(27.0) * dz, slope[None, :] * dz)
        theta[t] = ath_lin + (ten ** ((level[None, :] + shiftd[bins][None, :] + sf) / ten)).astype(dtype).sum(axis=1, dtype=dtype)
    return theta, count, margin


def threshold_db(theta):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(theta)


def loss_scale(psd_max):
    return 10.0 ** 9.6 / 10.0 ** (float(psd_max) / 10.0) * (8.0 / 3.0) / N ** 2


def loss_grad(delta, theta, psd_max, dtype=np.float64, detail=False):
    """delta [n], theta [T, 1025] linear, psd_max -> (loss, grad [n]); ``detail`` adds P [T, 1025]."""
    delta = np.asarray(delta, dtype=dtype)
    x = stft(delta, dtype)
    t = len(x)
    c = dtype(loss_scale(psd_max))
    theta = np.asarray(theta, dtype=dtype)
    p = (c * (x.real ** 2 + x.imag ** 2)).astype(dtype)
    over = p > theta
    loss = dtype(np.where(over, p - theta, dtype(0.0)).sum(dtype=dtype) / dtype(K * t))
    z = (np.where(over, dtype(loss_scale(psd_max) / (K * t)), dtype(0.0)) * x).astype(x.dtype)
    z[:, 0] *= 2
    z[:, K - 1] *= 2
    gt = (sfft.irfft(z, n=N, axis=1) * dtype(N)).astype(dtype) * hann(dtype)
    g = np.zeros(len(delta), dtype=dtype)
    for i in range(t):  # ascending frames, the order of the overlap-add
        g[HOP * i:HOP * i + N] += gt[i]
    return (loss, g, p) if detail else (loss, g)


def step(delta, x0, g_net, g_theta, alpha, eps, lr, use_sign, lo, hi):
    """The attack's step on float32 rows [B, n]; alpha, eps [B]."""
    f = np.float32
    t = g_net.astype(f)
    if g_theta is not None:
        t = t + alpha.astype(f)[:, None] * g_theta.astype(f)
    if use_sign:
        t = np.sign(t)
    e = eps.astype(f)[:, None]
    d = np.clip(delta.astype(f) - f(lr) * t, -e, e)
    xa = np.clip(x0.astype(f) + d, f(lo), f(hi))
    return xa - x0.astype(f), xa


# ---- seeded inputs shared by the CPU and the GPU tests ----
def clips(n, sr, batch, seed=0):
    """``batch`` different tone-plus-noise clips [batch, n] float32 in (-1, 1); with batch > 1 row 1 is all zeros."""
    rng = np.random.default_rng(1000 * seed + n + sr)
    t = np.arange(n) / sr
    out = np.zeros((batch, n), dtype=np.float32)
    for u in range(batch):
        if batch > 1 and u == 1:
            continue
        w = np.zeros(n)
        for _ in range(5):
            w += rng.uniform(0.02, 0.2) * np.sin(2 * np.pi * rng.uniform(100.0, 0.45 * sr) * t + rng.uniform(0, 2 * np.pi))
        w += rng.uniform(0.002, 0.02) * rng.standard_normal(n)
        out[u] = (w * np.minimum(1.0, 0.5 + t * sr / n)).astype(np.float32)
    return out


def noise(n, batch, seed=0):
    return np.random.default_rng(77 + seed + n).standard_normal((batch, n)).astype(np.float32)


def sawtooth(seed):
    """A synthetic PSD frame: 511 peaks of distinct seeded heights in [40, 95] dB at the odd bins 1 .. 1021 over 0 dB valleys."""
    rng = np.random.default_rng(seed)
    h = 40.0 + 55.0 * rng.permutation(511) / 510.0 + rng.uniform(-0.04, 0.04, 511)
    v = np.zeros(K, dtype=np.float32)
    v[1:1023:2] = np.clip(h, 40.0, 95.0).astype(np.float32)
    return v


SAW_SEED = {"bin": 1, "position": 1}
AMPLITUDES = (1e-3, 1e-2, 5e-2)
