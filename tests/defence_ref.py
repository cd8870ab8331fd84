"""NumPy restatement of the input-transformation defences (include/lipasr.h, lipasr_defence_apply / lipasr_defence_vjp),
independent of the library.

    apply(x, stages, n_valid, dtype)      [B, n] -> [B, n]
    vjp(x, g, stages, n_valid, dtype)     [B, n], [B, n] -> [B, n]

``stages`` is the public form, [("median", 5), ("fir", taps), ("quantize", 8)].  dtype=np.float64 is the truth: plain float64 sums.
dtype=np.float32 is the arithmetic of the library, bit for bit: the median and the quantiser are exact, and every step of a FIR
chain is one correctly rounded fused multiply-add (``fma32``), vectorised over the row.  Every stage works on rows padded with PAD
zeros on either side and masked to the clip, so a window never needs a special case."""
import numpy as np

PAD = 128
TILE = 1024  # positions of a workgroup

# name -> stages without their taps: ("fir", count) stands for count random taps (taps_for)
CHAINS = {
    "median5": [("median", 5)],
    "fir31": [("fir", 31)],
    "quantize8": [("quantize", 8)],
    "quantize2": [("quantize", 2)],
    "median15-fir255": [("median", 15), ("fir", 255)],
    "quantize4-median7": [("quantize", 4), ("median", 7)],
    "median3-fir101-quantize8": [("median", 3), ("fir", 101), ("quantize", 8)],
    "fir9-median5-quantize16-median3": [("fir", 9), ("median", 5), ("quantize", 16), ("median", 3)],
    "cap-median15-fir255-fir245-quantize4": [("median", 15), ("fir", 255), ("fir", 245), ("quantize", 4)],  # 7 + 127 + 122 = 256
}
# (chain, clips, n): every n of {1, 5, tile - 1, tile, tile + 1, 2 tile + 3} and every clips of {1, 3, 33} for each stage alone and
# for the chain at the cap, the tile edges for the others
_NS = (1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
_CLIPS = (33, 3, 1, 3, 33, 3)
CASES = [(c, b, n) for c in ("median5", "fir31", "quantize8", "cap-median15-fir255-fir245-quantize4") for b, n in zip(_CLIPS, _NS)]
CASES += [("median15-fir255", 3, TILE + 1), ("median15-fir255", 1, 2 * TILE + 3), ("quantize4-median7", 33, TILE - 1),
          ("quantize2", 3, 5), ("median3-fir101-quantize8", 3, TILE), ("median3-fir101-quantize8", 33, 2 * TILE + 3),
          ("fir9-median5-quantize16-median3", 1, TILE + 1), ("fir9-median5-quantize16-median3", 3, 2 * TILE + 3)]
ids = lambda c: f"{c[0]}-{c[1]}x{c[2]}"


def taps_for(count, seed=0):
    """``count`` taps ~ N(0, 1) / sqrt(count), float32 (not a low-pass: the loss of any tap shows)."""
    return (np.random.default_rng(7000 + 10 * count + seed).standard_normal(count) / np.sqrt(count)).astype(np.float32)


def stages_of(name):
    return [(k, taps_for(a, i) if k == "fir" else a) for i, (k, a) in enumerate(CHAINS[name])]


def inputs(clips, n, levels=False, seed=0):
    """x, g [clips, n] float32.  levels=False: x ~ U(-1.2, 1.2) (some samples beyond a quantiser's clamp), without -0.
    levels=True: x drawn from {-0.5, -0.25, 0, 0.25, 0.5} with every other zero a -0, so that ties are everywhere, also against the
    padding zeros, and the position has to decide."""
    rng = np.random.default_rng(100000 * seed + 31 * clips + n)
    if levels:
        x = rng.choice(np.array([-0.5, -0.25, 0.0, 0.25, 0.5], dtype=np.float32), size=(clips, n))
        flat = x.reshape(-1)
        zeros = np.flatnonzero(flat == 0)
        flat[zeros[::2]] = np.float32(-0.0)
    else:
        x = rng.uniform(-1.2, 1.2, (clips, n)).astype(np.float32)
        x[x == 0] = np.float32(0.5)
    g = rng.uniform(-1, 1, (clips, n)).astype(np.float32)
    return x, g


def mixed_lengths(clips, n):
    """0, 1, 37, n, n + 5 and -2 dealt over the clips (the callee clamps to [0, n]), the full length first so that one clip has it."""
    vals = (n, 0, 1, 37, n + 5, -2)
    return np.array([vals[i % len(vals)] for i in range(clips)], dtype=np.int32)


def clamp_lengths(n_valid, b, n):
    if n_valid is None:
        return np.full(b, n, dtype=np.int64)
    nv = np.clip(np.asarray(n_valid, dtype=np.int64), 0, n)
    assert nv.shape == (b,)
    return nv


def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, for float32 a, b, c given in any float type.  The product is exact in float64; the sum
    is rounded to float64 TO ODD (Knuth's two-sum gives the error, which says whether and where the exact value lies off the
    rounded one), and a value rounded to odd at 53 bits rounds to 24 bits as the exact value would."""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _pad(x, nv, dtype):
    b, n = x.shape
    out = np.zeros((b, n + 2 * PAD), dtype=dtype)
    m = np.arange(n)[None, :] < nv[:, None]
    out[:, PAD:PAD + n] = np.where(m, x, 0)  # np.where keeps the sign of a -0 inside the clip
    return out


def _windows(u, h):
    """[B, n + 2 PAD] -> [B, n, 2 h + 1]: the window of every position of the row."""
    n = u.shape[1] - 2 * PAD
    return np.lib.stride_tricks.sliding_window_view(u[:, PAD - h:PAD + n + h], 2 * h + 1, axis=1)


def _median_pick(u, k):
    """j [B, n]: which element of its window every position selects.  A stable sort by value IS the order (value, position): -0
    and +0 compare equal, so the earlier position comes first."""
    w = _windows(u, (k - 1) // 2)
    return np.argsort(w, axis=2, kind="stable")[:, :, (k - 1) // 2], w


def _forward(x, stages, nv, dtype):
    """The padded input of every stage and the routing of every stage (median: selected position per output, -1 outside the clip
    or where a padding zero was selected; quantize: idle mask), then the padded output."""
    b, n = x.shape
    inside = np.arange(n)[None, :] < nv[:, None]
    u = _pad(np.asarray(x, dtype=dtype), nv, dtype)
    routes = []
    for kind, arg in stages:
        out = np.zeros_like(u)
        if kind == "median":
            h = (int(arg) - 1) // 2
            j, w = _median_pick(u, int(arg))
            val = np.take_along_axis(w, j[:, :, None], axis=2)[:, :, 0]
            s = np.arange(n)[None, :] - h + j
            routes.append(np.where(inside & (s >= 0) & (s < nv[:, None]), s, -1))
        elif kind == "fir":
            taps = np.asarray(arg, dtype=np.float32)
            c = (len(taps) - 1) // 2
            val = np.zeros((b, n), dtype=dtype)
            for k in range(len(taps)):  # out[t] += h[k] x[t + c - k], ascending k
                xs = u[:, PAD + c - k:PAD + c - k + n]
                val = fma32(taps[k], xs, val) if dtype == np.float32 else val + np.float64(taps[k]) * xs
            routes.append(None)
        elif kind == "quantize":
            q = dtype(2 ** (int(arg) - 1))
            r = np.rint(u[:, PAD:PAD + n] * q)
            routes.append(inside & (r >= -q) & (r <= q - 1))
            val = np.clip(r, -q, q - 1) / q
        else:
            raise ValueError(kind)
        out[:, PAD:PAD + n] = np.where(inside, val, 0)
        u = out
    return u, routes


def apply(x, stages, n_valid=None, dtype=np.float64):
    x = np.asarray(x)
    nv = clamp_lengths(n_valid, *x.shape)
    u, _ = _forward(x, stages, nv, dtype)
    return np.ascontiguousarray(u[:, PAD:PAD + x.shape[1]])


def vjp(x, g, stages, n_valid=None, dtype=np.float64):
    x, g = np.asarray(x), np.asarray(g)
    b, n = x.shape
    nv = clamp_lengths(n_valid, b, n)
    inside = np.arange(n)[None, :] < nv[:, None]
    _, routes = _forward(x, stages, nv, dtype)
    gu = _pad(np.asarray(g, dtype=dtype), nv, dtype)
    for (kind, arg), route in zip(stages[::-1], routes[::-1]):
        if kind == "median":
            h = (int(arg) - 1) // 2
            sel = np.full((b, n + 2 * PAD), -1, dtype=np.int64)
            sel[:, PAD:PAD + n] = route
            val = np.zeros((b, n), dtype=dtype)
            pos = np.arange(n)[None, :]
            for d in range(-h, h + 1):  # output t = s + d, in ascending t
                hit = sel[:, PAD + d:PAD + d + n] == pos
                val = np.where(hit, (val + gu[:, PAD + d:PAD + d + n]).astype(dtype), val)
        elif kind == "fir":
            taps = np.asarray(arg, dtype=np.float32)
            c = (len(taps) - 1) // 2
            val = np.zeros((b, n), dtype=dtype)
            for k in range(len(taps)):  # gx[s] += h[k] g[s - c + k], ascending k
                gs = gu[:, PAD - c + k:PAD - c + k + n]
                val = fma32(taps[k], gs, val) if dtype == np.float32 else val + np.float64(taps[k]) * gs
        else:
            val = np.where(route, gu[:, PAD:PAD + n], 0)
        out = np.zeros_like(gu)
        out[:, PAD:PAD + n] = np.where(inside, val, 0)
        gu = out
    return np.ascontiguousarray(gu[:, PAD:PAD + n])


def native(stages):
    """``stages`` as the (kind, arg, taps) triples lipasr._native.defence_apply_host takes."""
    code = {"median": 0, "fir": 1, "quantize": 2}
    return [(code[k], len(a) if k == "fir" else int(a), np.asarray(a, dtype=np.float32) if k == "fir" else None) for k, a in stages]
