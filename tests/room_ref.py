"""NumPy restatement of the over-the-air channel (include/lipasr.h, lipasr_room_apply / lipasr_room_vjp) and of
lipasr.room.synthetic_rirs, independent of both.

    apply(x, rirs, n_valid, dtype)          [B, n] -> [B * R, n]
    vjp(g, rirs, n_valid, scale, dtype)     [B * R, n] -> [B, n]

dtype=np.float64 is the truth.  dtype=np.float32 runs every sum sequentially in (j, k) order with one rounded multiply-add per
tap -- the product of two floats is exact in float64, the sum with the float32 accumulator is rounded to float64 and then to
float32 -- vectorised over the time axis: ``taps`` NumPy operations per room.  That is the arithmetic of the library's host twins,
bit for bit."""
import numpy as np

# (clips, R, taps, n): the issue's ten, then one shape on each side of every edge of the one kernel instance there is -- 32 clips
# per tile, 128 output times per workgroup (32 per wavefront), 64 signal positions per staged chunk -- and the largest response
SHAPES = [(1, 1, 1, 1), (3, 3, 2, 37), (1, 1, 31, 255), (3, 1, 32, 256), (33, 3, 33, 257), (32, 16, 127, 1000), (3, 3, 257, 4099),
          (2, 2, 2048, 37), (3, 3, 2048, 22050), (33, 2, 64, 16000),
          (31, 1, 63, 127), (32, 2, 64, 128), (33, 1, 65, 129), (1, 2, 8192, 200)]
ids = lambda s: "x".join(str(v) for v in s)


def inputs(shape):
    """x [clips, n], g [clips * R, n] ~ U(-1, 1) and taps [R, taps] ~ N(0, 1) (not decaying: the loss of any tap shows)."""
    clips, r, taps, n = shape
    rng = np.random.default_rng(1000 * taps + n)
    x = rng.uniform(-1, 1, (clips, n)).astype(np.float32)
    g = rng.uniform(-1, 1, (clips * r, n)).astype(np.float32)
    return x, g, rng.standard_normal((r, taps)).astype(np.float32)


def clamp_lengths(n_valid, b, n):
    if n_valid is None:
        return np.full(b, n, dtype=np.int64)
    nv = np.clip(np.asarray(n_valid, dtype=np.int64), 0, n)
    assert nv.shape == (b,)
    return nv


def _mask(nv, n):
    return np.arange(n)[None, :] < nv[:, None]


def apply(x, rirs, n_valid=None, dtype=np.float64):
    """out[b * R + j][t] = sum_{k <= min(t, taps - 1)} rirs[j][k] * x[b][t - k] for t < nv_b, 0 from nv_b on."""
    x = np.asarray(x)
    rirs = np.asarray(rirs)
    (b, n), (r, taps) = x.shape, rirs.shape
    nv = clamp_lengths(n_valid, b, n)
    m = _mask(nv, n)
    xm = np.where(m, x, 0).astype(np.float64)  # x is read only below nv; above, the outputs are dropped anyway
    h = rirs.astype(np.float64)
    acc = np.zeros((b, r, n), dtype=dtype)
    buf = np.empty((b, r, n), dtype=np.float64)
    top = int(nv.max()) if b else 0  # nothing at or above the longest clip is read or kept
    for k in range(min(taps, top)):
        # out[:, :, t] += h[:, k] * x[:, t - k] for k <= t < top: exact product, float64 sum, then rounded to dtype on assignment
        term = np.multiply(h[None, :, k, None], xm[:, None, :top - k], out=buf[:, :, :top - k])
        term += acc[:, :, k:top]
        acc[:, :, k:top] = term
    return np.where(m[:, None, :], acc, 0).astype(dtype).reshape(b * r, n)


def vjp(g, rirs, n_valid=None, scale=1.0, dtype=np.float64):
    """gx[b][s] = scale * sum_j sum_{k < taps, s + k < nv_b} rirs[j][k] * g[b * R + j][s + k] for s < nv_b, 0 from nv_b on."""
    g = np.asarray(g)
    rirs = np.asarray(rirs)
    r, taps = rirs.shape
    n = g.shape[1]
    b = g.shape[0] // r
    nv = clamp_lengths(n_valid, b, n)
    m = _mask(nv, n)
    gm = np.where(m[:, None, :], g.reshape(b, r, n), 0).astype(np.float64)
    h = rirs.astype(np.float64)
    acc = np.zeros((b, n), dtype=dtype)
    buf = np.empty((b, n), dtype=np.float64)
    top = int(nv.max()) if b else 0  # nothing at or above the longest clip is read or kept
    for j in range(r):
        for k in range(min(taps, top)):
            term = np.multiply(h[j, k], gm[:, j, k:top], out=buf[:, :top - k])
            term += acc[:, :top - k]
            acc[:, :top - k] = term
    if dtype == np.float32:
        out = np.float32(scale) * acc
    else:
        out = float(np.float32(scale)) * acc
    return np.where(m, out, 0).astype(dtype)


def synthetic_rirs(count, sr=22050, taps=2048, t60=(0.15, 0.5), drr_db=(0.0, 12.0), seed=0):
    """h[0] = 1; h[k] = a eps_k 10^(-3 k / (t60 sr)) with sum_{k>0} h[k]^2 = 10^(-drr_db / 10).  Draws, in this order, from
    Generator(PCG64(seed)): t60 per room (if a range), drr_db per room (if a range), eps [count, taps - 1]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.full(count, float(t60)) if np.ndim(t60) == 0 else rng.uniform(t60[0], t60[1], size=count)
    d = np.full(count, float(drr_db)) if np.ndim(drr_db) == 0 else rng.uniform(drr_db[0], drr_db[1], size=count)
    eps = rng.standard_normal((count, taps - 1))
    out = np.zeros((count, taps))
    for j in range(count):
        tail = eps[j] * 10.0 ** (-3.0 * np.arange(1, taps) / (t[j] * sr))
        e = np.sum(tail * tail)
        out[j, 0] = 1.0
        out[j, 1:] = tail * np.sqrt(10.0 ** (-d[j] / 10.0) / (e if e > 0 else 1.0))
    return out.astype(np.float32)


def ragged_lengths(clips, n):
    """The n_valid vectors of the ragged cases: 0, 1, 37 (where <= n), n and n + 5 (clamped by the callee) dealt over the clips,
    in as many vectors as it takes for every value to appear."""
    vals = [v for v in (0, 1, 37, n, n + 5) if v <= n or v == n + 5]
    cases = []
    for first in range(0, len(vals), max(clips, 1)):
        cases.append(np.array([vals[(first + i) % len(vals)] for i in range(clips)], dtype=np.int32))
    return cases
