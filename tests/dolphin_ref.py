"""Oracle restatement of the DolphinAttack chain (include/lipasr.h, "DolphinAttack") with SciPy, for tests only: the product
never imports it.  MATLAB is absent, so this restates dolphin_attack.m's calls from their documentation:
butter(10, [100 7000]/8000) as second-order sections, resample(x, 12, 1) / resample(x, 1, 12) with the default filter
(firls x kaiser(5), n = 10), and the two peak normalisations around the AM step.  The centred interpolator and decimator are
plain convolutions that skip the stuffed zeros (scipy.signal.upfirdn on the filter as it is, so that MATLAB's zero-prepend and
delay rule, restated with the same routine, adds only zero terms and compares exactly).  ``chain`` runs in float64 or, as the
yardstick of the device's fp32 arithmetic, with every array and every intermediate in float32."""
import numpy as np
from scipy import signal

SR, RATIO, SR_OUT = 16000, 12, 192000
HALF = 10 * RATIO  # the resampling filter reaches 10 slow samples to each side


def sos():
    return signal.butter(10, [2 * 100 / SR, 2 * 7000 / SR], "bandpass", output="sos")


def ba():
    """The transfer-function form the script itself calls filter() with (quirk 1: unstable in double precision)."""
    return signal.butter(10, [2 * 100 / SR, 2 * 7000 / SR], "bandpass")


def resample_filter(p, q):
    """MATLAB resample(x, p, q)'s default filter: n = 10, beta = 5."""
    m = max(p, q)
    fc = 1.0 / (2 * m)
    L = 2 * 10 * m + 1
    h = signal.firls(L, [0, 2 * fc, 2 * fc, 1], [1, 1, 0, 0]) * np.kaiser(L, 5)
    return p * h / h.sum()


def up_centred(v, h):
    """u[k] = sum_j h[k + 120 - 12 j] v[j], k < 12 n."""
    return signal.upfirdn(h.astype(v.dtype), v, RATIO, 1)[HALF:HALF + RATIO * len(v)]


def down_centred(w, h):
    """r[i] = sum_k h[12 i + 120 - k] w[k], i < len(w) / 12."""
    return signal.upfirdn(h.astype(w.dtype), w, 1, RATIO)[HALF // RATIO:HALF // RATIO + len(w) // RATIO]


def matlab_resample(x, p, q):
    """resample(x, p, q) by MATLAB's own rule: prepend zeros to the filter so that the delay is a whole number of output
    samples, upfirdn, drop the delay, keep ceil(n p / q) samples."""
    h = resample_filter(p, q)
    lhalf = (len(h) - 1) // 2
    nz = q - lhalf % q
    h = np.concatenate([np.zeros(nz), h])
    lhalf += nz
    delay = lhalf // q
    ly = -(-len(x) * p // q)
    y = signal.upfirdn(h, x, p, q)
    return y[delay:delay + ly]


def carrier(n_out, carrier_hz, dtype):
    ph = (np.arange(n_out, dtype=np.int64) * int(carrier_hz)) % SR_OUT
    if dtype == np.float32:
        return np.cos((np.float32(2 * np.pi) * ph.astype(np.float32) / np.float32(SR_OUT)).astype(np.float32)).astype(np.float32)
    return np.cos(2 * np.pi * ph / SR_OUT)


def record(s, a1, a2, dtype=np.float64):
    s = np.asarray(s, dtype=dtype)
    w = dtype(a1) * s + dtype(a2) * s * s
    return down_centred(w, resample_filter(1, RATIO))


def chain(x, dtype=np.float64, carrier_level=0.001, carrier_hz=30000, a1=1.0, a2=0.5):
    """-> (v, s, peaks, r): the band-passed voice [n], the ultrasound [12 n], (m1, m2), the recorded clip [n]."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype)
    v = signal.sosfilt(sos().astype(dtype), x)
    assert v.dtype == dtype, v.dtype
    u = up_centred(v, resample_filter(RATIO, 1))
    m1 = np.abs(u).max()
    uh = u / m1 if m1 > 0 else np.zeros_like(u)
    sp = (uh + dtype(carrier_level)) * carrier(len(u), carrier_hz, dtype)
    m2 = np.abs(sp).max()
    s = sp / m2 if m2 > 0 else np.zeros_like(sp)
    r = record(s, a1, a2, dtype)
    assert s.dtype == dtype and r.dtype == dtype
    return v, s, np.array([m1, m2], dtype=dtype), r


def chirp(n, seed=1):
    """0.3 sin(2 pi (200 t + 1500 t^2)) hanning + 0.02 noise."""
    t = np.arange(n) / SR
    return 0.3 * np.sin(2 * np.pi * (200 * t + 1500 * t * t)) * np.hanning(n) + 0.02 * np.random.default_rng(seed).standard_normal(n)


def voiced(n, f0=140.0, seed=2):
    """A harmonic stack with a slow envelope: twelve harmonics of f0 falling off as 1 / h."""
    t = np.arange(n) / SR
    rng = np.random.default_rng(seed)
    s = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 13))
    return 0.25 * s / np.abs(s).max() * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))


def quiet_noise(n, seed=3):
    return 1e-3 * np.random.default_rng(seed).standard_normal(n)


def demod_correlation(r, v):
    """Correlation of the recorded clip (mean removed) with the voice."""
    r = np.asarray(r, dtype=np.float64) - np.mean(r)
    v = np.asarray(v, dtype=np.float64)
    return float(np.dot(r, v) / (np.linalg.norm(r) * np.linalg.norm(v)))
