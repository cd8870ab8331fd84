"""Square Attack without a GPU: lipasr_square_init_host / lipasr_square_step_host (the CPU-side pin of the counters and of the
arithmetic the device kernels share with them) against the NumPy restatement of tests/square_ref.py bit for bit, the step's
conventions on hand-made logits, the statistics of the draws, every refusal of the ABI, the surface of lipasr.square and
lipasr.attacks.AutoAttack, and a known answer on a linear model from the restatement alone.

Bounds.  Everything the kernels compute is integer arithmetic, one fp32 add, two clamps and one fp32 subtract, and the
restatement does the same in NumPy float32 and Python integers: every comparison is of bits.  The two statistics are 5-sigma
binomial intervals."""
import ctypes as C
import math

import numpy as np
import pytest

import square_ref as R

SHAPES = [(1, 1, 1), (1, 1, 5), (2, 3, 7), (3, 20, 44), (2, 1, 1030), (2, 20, 101)]
FULL = 1 << 24
ids = lambda s: "x".join(map(str, s))


def _rows(B, n, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal((B, n))).astype(np.float32)


def _logits(B, C_, seed):
    return np.random.default_rng(seed + 500).standard_normal((B, C_)).astype(np.float32)


def _N():
    from lipasr import _native as N

    return N


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def host_state(x0, height, width, restart, seed, eps, **kw):
    best, cand, win = _N().square_init_host(x0, height, width, restart, seed, eps, **kw)
    return dict(x_best=best, x_cand=cand, win=win, loss_best=np.zeros(len(x0), dtype=np.float32), done=np.zeros(len(x0), dtype=np.int32))


def host_step(st, logits, labels, x0, height, width, wh, ww, pq, restart, it, seed, eps, **kw):
    _N().square_step_host(logits, labels, x0, height, width, wh, ww, pq, restart, it, seed, eps, x_best=st["x_best"], x_cand=st["x_cand"],
                          loss_best=st["loss_best"], done=st["done"], win=st["win"], **kw)


def ref_state(x0, height, width, restart, seed, eps, n_valid=None, clip0=0, lo=-np.inf, hi=np.inf):
    st = R.init(x0, height, width, restart, seed, eps, n_valid, clip0, lo, hi)
    st["loss_best"], st["done"] = np.zeros(len(x0), dtype=np.float32), np.zeros(len(x0), dtype=np.int32)
    return st


def assert_state(got, want, what):
    for k in ("x_best", "x_cand", "win", "loss_best", "done"):
        assert same(got[k], want[k]), f"{what}: {k} differs"


def chain(shape, seed, eps, iters, n_valid=None, clip0=0, lo=-np.inf, hi=np.inf, restart=1, p=0.3, rows=slice(None), check=True):
    """``iters`` steps of the host twins next to the restatement, on random logits; returns the host state."""
    B, height, width = shape
    x0 = _rows(B, height * width, seed)[rows]
    nv = None if n_valid is None else np.asarray(n_valid, dtype=np.int32)[rows]
    labels = (np.arange(B, dtype=np.int32) % 3)[rows]
    kw_h = dict(n_valid=nv, clip0=clip0, clip_lo=lo, clip_hi=hi)
    got = host_state(x0, height, width, restart, seed, eps, **kw_h)
    want = ref_state(x0, height, width, restart, seed, eps, nv, clip0, lo, hi)
    if check:
        assert_state(got, want, f"{ids(shape)} init")
    for it in range(iters):
        z = _logits(B, 4, seed + it)
        z[np.arange(B), np.arange(B) % 3] += 4.0 if it < iters - 3 else 0.0  # rows stay in their class until the last three queries
        z = z[rows]
        wh, ww = R.square_window(p, height, width)
        last = it + 1 == iters
        host_step(got, z, labels, x0, height, width, wh, ww, R.p_q(p), restart, it, seed, eps, last=last, **kw_h)
        if check:
            R.step(want, z, labels, x0, height, width, wh, ww, R.p_q(p), restart, it, seed, eps, nv, False, last, clip0, lo, hi)
            assert_state(got, want, f"{ids(shape)} step {it}")
            inside = np.zeros((len(x0), height, width), dtype=bool)
            for b, (r, c, h, w) in enumerate(got["win"]):
                inside[b, r:r + h, c:c + w] = True
            differs = (got["x_best"].view(np.uint32) != got["x_cand"].view(np.uint32)).reshape(inside.shape)
            assert not (differs & ~inside).any(), "x_cand differs from x_best outside win"
            if last:
                assert not differs.any() and not got["win"].any()
    return got, x0


# ---------------------------------------------------------------------------------------------------------------- host twins
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_host_twins_match_the_restatement(shape):
    B, height, width = shape
    seed = 11 + sum(shape)
    got, x0 = chain(shape, seed, 0.1, 12)
    # every perturbed element is x0 +- eps in float32
    e = np.float32(0.1)
    assert (np.isin(got["x_best"].view(np.uint32), (x0 + e).view(np.uint32)) | np.isin(got["x_best"].view(np.uint32), (x0 - e).view(np.uint32))).all()
    for k in ("x_best",):
        assert ((got[k] == x0 + e) | (got[k] == x0 - e)).all()
    chain(shape, seed, 0.25, 8, lo=-0.2, hi=0.35, restart=255)
    chain(shape, seed, 0.0, 3)
    # one stripe sign per column
    st = host_state(x0, height, width, 0, seed, 0.1)
    up = (st["x_best"] == x0 + e).reshape(B, height, width)
    assert (up == up[:, :1, :]).all()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] == 1], ids=ids)
def test_n_valid_on_the_strips(shape):
    B, _, n = shape
    values = [0, 1, 5, n - 1, n, n + 3, -2]
    for s in range(0, len(values), B):
        nv = np.array((values[s:] + values)[:B], dtype=np.int32)
        got, x0 = chain(shape, 5, 0.1, 10, n_valid=nv, p=0.4)
        clamped = np.clip(nv, 0, n)
        for b in range(B):
            assert same(got["x_best"][b, clamped[b]:], x0[b, clamped[b]:]) and same(got["x_cand"][b, clamped[b]:], x0[b, clamped[b]:])
    # the segment is a share of the clip's own samples
    nvs = np.array([max(n // 2, 1)] * B, dtype=np.int32)
    st = host_state(_rows(B, n, 1), 1, n, 0, 3, 0.1, n_valid=nvs)
    z = np.tile(np.array([[1.0, 0.0, 0.0]], dtype=np.float32), (B, 1))  # margin 1: no row is done, every row gets a proposal
    host_step(st, z, np.zeros(B, dtype=np.int32), _rows(B, n, 1), 1, n, 1, 1, R.p_q(0.5), 0, 0, 3, 0.1, n_valid=nvs)
    want_w = min(max((int(nvs[0]) * R.p_q(0.5) + (1 << 23)) >> 24, 1), int(nvs[0]))
    assert (st["win"][:, 3] == want_w).all() and (st["win"][:, 1] + st["win"][:, 3] <= nvs).all()


def test_n_valid_needs_a_strip():
    N = _N()
    x0 = _rows(2, 21, 0)
    with pytest.raises(ValueError, match="n_valid with height 3"):
        N.square_init_host(x0, 3, 7, 0, 0, 0.1, n_valid=np.array([3, 4], dtype=np.int32))
    st = host_state(x0, 3, 7, 0, 0, 0.1)
    with pytest.raises(ValueError, match="n_valid with height 3"):
        host_step(st, _logits(2, 3, 0), np.zeros(2, dtype=np.int32), x0, 3, 7, 1, 1, 0, 0, 0, 0, 0.1, n_valid=np.array([3, 4], dtype=np.int32))


@pytest.mark.parametrize("shape", [(3, 20, 44), (3, 1, 1030)], ids=ids)
def test_draws_do_not_depend_on_the_chunk(shape):
    nv = None if shape[1] > 1 else [1030, 517, 64]
    whole, _ = chain(shape, 9, 0.1, 9, n_valid=nv, check=False)
    tail, _ = chain(shape, 9, 0.1, 9, n_valid=nv, clip0=1, rows=slice(1, None), check=False)
    for k in ("x_best", "x_cand", "win", "loss_best", "done"):
        assert same(tail[k], whole[k][1:]), k
    head, _ = chain(shape, 9, 0.1, 9, n_valid=nv, clip0=0, rows=slice(0, 1), check=False)
    assert same(head["x_best"], whole["x_best"][:1])
    # the row index, the restart and the seed are all part of the counter
    base = host_state(_rows(1, shape[1] * shape[2], 9), shape[1], shape[2], 0, 9, 0.1)["x_best"]
    for kw in (dict(clip0=1), dict(restart=1), dict(seed=10)):
        args = dict(restart=0, seed=9, clip0=0)
        args.update(kw)
        other = _N().square_init_host(_rows(1, shape[1] * shape[2], 9), shape[1], shape[2], args["restart"], args["seed"], 0.1, clip0=args["clip0"])[0]
        assert (other != base).mean() > 0.2, kw


# ---------------------------------------------------------------------------------------------------------------- conventions
def _tiny(B=1, n=6, eps=0.5):
    x0 = np.zeros((B, n), dtype=np.float32)
    return x0, host_state(x0, 1, n, 0, 1, eps)


def _go(st, x0, z, it, labels=None, **kw):
    B, n = x0.shape
    labels = np.zeros(B, dtype=np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    host_step(st, np.asarray(z, dtype=np.float32).reshape(B, -1), labels, x0, 1, n, 1, 2, R.p_q(0.3), 0, it, 1, 0.5, **kw)


def test_step_conventions_ties_and_strictness():
    x0, st = _tiny()
    _go(st, x0, [[2.0, 1.0, -1.0]], 0)
    assert st["loss_best"][0] == 1.0 and st["done"][0] == 0 and st["win"][0, 3] == 2  # margin 2 - 1; a proposal is out
    best0, cand1 = st["x_best"].copy(), st["x_cand"].copy()
    assert not same(best0, cand1)
    _go(st, x0, [[2.0, 1.0, 1.0]], 1)  # a tie with the best: strict, so the proposal is taken back
    assert st["loss_best"][0] == 1.0 and same(st["x_best"], best0)
    cand2 = st["x_cand"].copy()
    _go(st, x0, [[2.0, 1.5, 1.0]], 2)  # lower: accepted, the window moves into x_best
    assert st["loss_best"][0] == 0.5
    assert same(st["x_best"], cand2) and (st["x_best"] != best0).sum() <= 2  # x_best is the candidate that was asked about
    _go(st, x0, [[1.0, 1.0, 0.0]], 3)  # margin 0 is not negative: better, but not done
    assert st["loss_best"][0] == 0.0 and st["done"][0] == 0


def test_step_conventions_nan_done_last():
    x0, st = _tiny(B=3)
    nan = math.nan
    _go(st, x0, [[nan, 1.0, 0.0], [1.0, nan, 0.0], [3.0, 1.0, 0.0]], 0)
    assert np.isposinf(st["loss_best"][:2]).all() and st["loss_best"][2] == 2.0 and not st["done"].any()
    best = st["x_best"].copy()
    _go(st, x0, [[nan, nan, nan], [0.0, 1.0, nan], [0.0, 1.0, 0.0]], 1)  # a NaN never wins, not even against +inf
    assert np.isposinf(st["loss_best"][:2]).all() and same(st["x_best"][:2], best[:2])
    assert st["loss_best"][2] == -1.0 and st["done"][2] == 2  # it + 1: two queries
    assert not st["win"][2].any() and same(st["x_cand"][2], st["x_best"][2]) and st["win"][0, 3] == 2
    frozen = st["x_best"][2].copy()
    _go(st, x0, [[0.0, 1.0, 0.0], [5.0, 1.0, 0.0], [0.0, 9.0, 0.0]], 2)  # sticky: a done row keeps its loss, its point, its count
    assert st["loss_best"][2] == -1.0 and st["done"][2] == 2 and same(st["x_best"][2], frozen) and same(st["x_cand"][2], frozen)
    assert st["done"][0] == 3 and st["loss_best"][1] == 4.0 and st["done"][1] == 0
    _go(st, x0, [[0.0, 1.0, 0.0], [4.5, 1.0, 0.0], [0.0, 9.0, 0.0]], 3, last=True)  # LAST: bookkeeping, then no proposal anywhere
    assert st["loss_best"][1] == 3.5 and not st["win"].any() and same(st["x_cand"], st["x_best"])


def test_step_conventions_classes_targeted_labels():
    x0, st = _tiny(B=2)
    _go(st, x0, [[7.0], [-7.0]], 0)  # one class: +inf, never done
    assert np.isposinf(st["loss_best"]).all() and not st["done"].any()
    _go(st, x0, [[7.0], [-7.0]], 0, targeted=True)
    assert np.isposinf(st["loss_best"]).all()
    x0, st = _tiny(B=2)
    _go(st, x0, [[1.0, 3.0, 0.0], [4.0, 3.0, 0.0]], 0, labels=[0, 0], targeted=True)  # the class to reach: -(z_y - max other)
    assert st["loss_best"].tolist() == [2.0, -1.0] and st["done"].tolist() == [0, 1]
    x0, st = _tiny(B=2)
    _go(st, x0, [[1.0, 3.0, 0.0], [4.0, 3.0, 0.0]], 0, labels=[-1, 3])  # labels outside the classes: +inf, nothing read out of bounds
    assert np.isposinf(st["loss_best"]).all() and not st["done"].any()
    inf = math.inf
    x0, st = _tiny(B=2)
    _go(st, x0, [[inf, inf, 0.0], [-inf, 0.0, 1.0]], 0)  # inf - inf is a NaN: stored as +inf; -inf - 1 = -inf: done
    assert np.isposinf(st["loss_best"][0]) and np.isneginf(st["loss_best"][1]) and st["done"].tolist() == [0, 1]
    # nv == 0: bookkeeping only
    x0 = _rows(1, 6, 3)
    st = host_state(x0, 1, 6, 0, 1, 0.5, n_valid=np.zeros(1, dtype=np.int32))
    assert same(st["x_best"], x0) and same(st["x_cand"], x0)
    _go(st, x0, [[2.0, 1.0, 0.0]], 0, n_valid=np.zeros(1, dtype=np.int32))
    assert st["loss_best"][0] == 1.0 and not st["win"].any() and same(st["x_cand"], x0)


def test_a_nan_stays_and_the_clip_binds():
    x0 = np.array([[math.nan, 0.9, -0.9, 0.0]], dtype=np.float32)
    st = host_state(x0, 1, 4, 0, 1, 0.5, clip_lo=-1.0, clip_hi=1.0)
    assert np.isnan(st["x_best"][0, 0]) and np.abs(st["x_best"][0, 1:]).max() <= 1.0
    assert st["x_best"][0, 1] in (np.float32(1.0), np.float32(0.9) - np.float32(0.5)) and abs(st["x_best"][0, 3]) == 0.5
    assert same(st["x_best"], R.init(x0, 1, 4, 0, 1, 0.5, lo=-1.0, hi=1.0)["x_best"])


# ---------------------------------------------------------------------------------------------------------------- statistics
def test_window_statistics():
    """120 000 proposals (iterations 0 .. 119 999 of one 3 x 7 row with a 2 x 2 window, every one rejected by a constant logit row):
    the share of minus signs, and the share of each of the 2 x 6 corner positions, inside 5-sigma binomial intervals.  And
    2 x 20 x 1030 stripe signs likewise."""
    draws = 120_000
    corners = np.zeros((2, 6), dtype=np.int64)
    minus = 0
    for it in range(1, draws + 1):
        (r, c, h, w), m = R.draw(77, 4, 2, it, 3, 7, None, 2, 2, 0)
        assert (h, w) == (2, 2) and 0 <= r <= 1 and 0 <= c <= 5
        corners[r, c] += 1
        minus += m
    assert abs(minus / draws - 0.5) <= 5 * math.sqrt(0.25 / draws)
    q = 1.0 / 12
    assert (np.abs(corners / draws - q) <= 5 * math.sqrt(q * (1 - q) / draws)).all(), corners
    # the host twin draws what the restatement draws (a sample of the iterations above), through the ABI
    x0 = _rows(1, 21, 2)
    st = host_state(x0, 3, 7, 2, 77, 0.1, clip0=4)
    z, lab = np.array([[1.0, 0.0]], dtype=np.float32), np.zeros(1, dtype=np.int32)
    for it in list(range(0, 300)) + [1000, 65535, 119_998]:
        host_step(st, z, lab, x0, 3, 7, 2, 2, 0, 2, it, 77, 0.1, clip0=4)
        (r, c, h, w), m = R.draw(77, 4, 2, it + 1, 3, 7, None, 2, 2, 0)
        assert st["win"][0].tolist() == [r, c, h, w]
        assert st["x_cand"][0, r * 7 + c] == x0[0, r * 7 + c] + (np.float32(-0.1) if m else np.float32(0.1))
    signs = np.concatenate([R.stripe_signs(5, clip, r, 1030) for clip in range(20) for r in range(2)])
    assert abs(signs.mean() - 0.5) <= 5 * math.sqrt(0.25 / signs.size)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_abi_argument_checks_without_a_device():
    N = _N()
    assert N.lib.lipasr_version() >= 660 and all(N.has(f"lipasr_square_{k}") for k in ("init", "step", "init_host", "step_host"))
    assert len(N.lib.lipasr_square_init.argtypes) == 16 and len(N.lib.lipasr_square_init_host.argtypes) == 14
    assert len(N.lib.lipasr_square_step.argtypes) == 27 and len(N.lib.lipasr_square_step_host.argtypes) == 25
    inf = math.inf
    fake = C.c_void_p(8)
    buf = np.zeros(256, dtype=np.float32)
    at = lambda k: C.c_void_p(buf.ctypes.data + 4 * k)
    ints = np.zeros(64, dtype=np.int32)
    ip = C.c_void_p(ints.ctypes.data)
    P = dict(x0=at(0), x_best=at(50), x_cand=at(100), win=ip)  # 2 rows of 3 x 7: 42 floats per buffer

    def init(host, h=fake, nv=None, B=2, height=3, width=7, restart=0, eps=0.1, lo=-inf, hi=inf, **p):
        p = dict(P, **p)
        if host:
            return N.lib.lipasr_square_init_host(p["x0"], nv, B, height, width, 0, restart, 0, eps, lo, hi, p["x_best"], p["x_cand"], p["win"])
        return N.lib.lipasr_square_init(h, p["x0"], nv, B, height, width, 0, restart, 0, eps, lo, hi, p["x_best"], p["x_cand"], p["win"], None)

    def step(host, h=fake, nv=None, B=2, classes=3, height=3, width=7, wh=1, ww=1, pq=0, restart=0, it=0, flags=0, eps=0.1, lo=-inf, hi=inf,
             logits=at(200), labels=ip, loss=at(220), done=ip, **p):
        p = dict(P, **p)
        tail = (p["x_best"], p["x_cand"], loss, done, p["win"])
        if host:
            return N.lib.lipasr_square_step_host(logits, labels, p["x0"], nv, B, classes, height, width, wh, ww, pq, 0, 0, restart, it, flags,
                                                 0, eps, lo, hi, *tail)
        return N.lib.lipasr_square_step(h, logits, labels, p["x0"], nv, B, classes, height, width, wh, ww, pq, 0, 0, restart, it, flags, 0,
                                        eps, lo, hi, *tail, None)

    shared = ((dict(restart=256), "restart 256"), (dict(eps=-1.0), "eps -1"), (dict(eps=inf), "eps inf"), (dict(eps=math.nan), "eps"),
              (dict(lo=1.0, hi=-1.0), "clip range"), (dict(lo=math.nan), "clip range"), (dict(B=-1), "bad shape"), (dict(height=-1), "bad shape"),
              (dict(width=-3), "bad shape"), (dict(height=1 << 16, width=1 << 16), "rows of"), (dict(nv=ip), "n_valid with height 3"),
              (dict(x0=None), "a null pointer"), (dict(x_best=None), "a null pointer"), (dict(x_cand=None), "a null pointer"),
              (dict(win=None), "a null pointer"), (dict(x_best=at(100 + 41)), "x_best overlaps x_cand"),
              (dict(x_best=at(100 - 41)), "x_best overlaps x_cand"), (dict(x_best=at(41)), "x_best overlaps x0"),
              (dict(x_best=at(150), x_cand=at(1)), "x_cand overlaps x0"))
    only_step = ((dict(it=1 << 24), "it 16777216"), (dict(classes=0), "0 classes"), (dict(classes=33), "33 classes"),
                 (dict(wh=0), "window 0 x 1"), (dict(wh=4), "window 4 x 1"), (dict(ww=0), "window 1 x 0"), (dict(ww=8), "window 1 x 8"),
                 (dict(pq=FULL + 1), "p_q 16777217"), (dict(flags=2), "flags 2"), (dict(logits=None), "a null pointer"),
                 (dict(labels=None), "a null pointer"), (dict(loss=None), "a null pointer"), (dict(done=None), "a null pointer"))
    for fn, extra, name in ((init, (), "lipasr_square_init"), (step, only_step, "lipasr_square_step")):
        for host in (False, True):
            full = name + ("_host:" if host else ":")
            for kw, msg in shared + extra + (() if host else ((dict(h=None), "null handle"),)):
                assert fn(host, **kw) == N.EINVAL, (full, kw)
                assert msg in N.last_error() and N.last_error().startswith(full), (kw, N.last_error())
            for zero in (dict(B=0), dict(height=0), dict(width=0)):
                assert fn(host, x0=None, x_best=None, x_cand=None, win=None, **zero) == N.OK, (full, zero)
            assert fn(True) == N.OK  # the same arguments untouched are accepted (host side: it runs)
    with pytest.raises(ValueError, match="x_best overlaps x_cand"):  # through the NumPy wrapper
        one = np.zeros((2, 21), dtype=np.float32)
        N.square_init_host(np.zeros((2, 21), dtype=np.float32), 3, 7, 0, 0, 0.1, x_best=one, x_cand=one)


def test_square_attack_is_exported_and_checks_its_arguments():
    import inspect

    from lipasr import attack_eval as V, attacks as A, square as Z

    assert A.SquareAttack is Z.SquareAttack and callable(V.square_sweep) and callable(Z.square_init) and callable(Z.square_step)
    sig = inspect.signature(Z.SquareAttack.__init__)
    assert list(sig.parameters)[1:8] == ["estimator", "norm", "max_iter", "eps", "p_init", "nb_restarts", "batch_size"]
    for k, d in (("norm", np.inf), ("max_iter", 100), ("eps", 0.3), ("p_init", 0.8), ("nb_restarts", 1), ("batch_size", 128)):
        assert sig.parameters[k].default == d
    for k, d in (("shape", None), ("targeted", False), ("seed", 0), ("p_schedule", Z.square_p), ("check_every", 10)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d
    assert sig.parameters["clip_values"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (Z.SquareAttack, A.AutoAttack):
        assert list(inspect.signature(cls.generate_device).parameters)[1:] == ["xt", "yt", "lengths"]
        assert list(inspect.signature(cls.generate).parameters)[1:] == ["x", "y", "lengths"]
        with pytest.raises(TypeError):
            cls(object())
    sig = inspect.signature(A.AutoAttack.__init__)
    assert list(sig.parameters)[1:7] == ["estimator", "norm", "eps", "eps_step", "attacks", "batch_size"]
    for k, d in (("norm", np.inf), ("eps", 0.3), ("eps_step", 0.1), ("attacks", None), ("batch_size", 32)):
        assert sig.parameters[k].default == d
    for k, d in (("seed", 0), ("shape", None)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d
    assert "difference_logits_ratio" in A.AutoAttack.__doc__ and "LEFT OUT" in A.AutoAttack.__doc__ and "unpinned" in Z.SquareAttack.__doc__


def test_schedule_and_window():
    from lipasr import square as Z

    assert [Z.square_p(it, 10000, 0.8) for it in (0, 10, 11, 50, 51, 200, 201, 500, 501, 1000, 1001, 2000, 2001, 4000, 4001, 6000, 6001, 8000,
                                                  8001, 9999)] == \
        [0.8, 0.8, 0.4, 0.4, 0.2, 0.2, 0.1, 0.1, 0.05, 0.05, 0.025, 0.025, 0.0125, 0.0125, 0.00625, 0.00625, 0.003125, 0.003125, 0.0015625,
         0.0015625]
    assert Z.square_p(1, 100, 0.8) == 0.2 and Z.square_p(0, 100, 0.8) == 0.8 and Z.square_p(99, 100, 1.0) == 1.0 / 512  # rescaled: 100, 9900
    for it in range(0, 500, 7):
        assert Z.square_p(it, 500, 0.3) == R.square_p(it, 500, 0.3)
    assert Z.square_window(0.8, 20, 44) == (20, 27) and Z.square_window(0.05, 20, 44) == (7, 7) and Z.square_window(1e-9, 20, 44) == (1, 1)
    assert Z.square_window(1.0, 20, 101) == (20, 45) and Z.square_window(0.1, 1, 22050) == (1, 2205) and Z.square_window(0.0, 1, 5) == (1, 1)
    assert Z.square_window(1.0, 1, 4) == (1, 4)
    for p in (0.8, 0.1, 0.003):
        for hw in ((20, 44), (1, 1030), (3, 7)):
            assert Z.square_window(p, *hw) == R.square_window(p, *hw)
        assert Z.square_p_q(p) == R.p_q(p)
    assert Z.square_p_q(1.0) == FULL and Z.square_p_q(0.0) == 0 and Z.square_p_q(7.0) == FULL
    with pytest.raises(ValueError):
        Z.square_window(0.5, 0, 4)


def test_menu_accepts_square_and_auto(tmp_path):
    """attack_eval.main takes --attack black --kind square and --attack white --kind auto over either domain and goes on to load the
    dataset."""
    from lipasr import attack_eval as V

    missing = str(tmp_path) + "/missing/"
    for over in ("mfcc", "audio"):
        with pytest.raises(FileNotFoundError):
            V.main(["--attack", "black", "--kind", "square", "--over", over, "--points", "1", "--max-iter", "5", "--path", missing])
        for norm in ("inf", "2"):
            with pytest.raises(FileNotFoundError):
                V.main(["--attack", "white", "--kind", "auto", "--over", over, "--norm", norm, "--points", "1", "--path", missing])
    with pytest.raises(ValueError, match="--kind auto runs in --norm inf or 2"):
        V.main(["--attack", "white", "--kind", "auto", "--norm", "1", "--path", missing])


# ---------------------------------------------------------------------------------------------------------------- known answer
def test_known_answer_on_a_linear_model():
    """Two classes, a 1 x 4 strip, logits z = x W with every weight difference w_0 - w_1 positive, label 0, p_init = 1.0 and a
    constant schedule: every window is the whole row (round(1.0 * 4) = 4), so a proposal is all +eps or all -eps.  The margin
    (w_0 - w_1) . x is smallest at x0 - eps: the first proposal whose sign bit is minus reaches
    fl32-evaluated margin(x0 - eps) = margin(x0) - eps ||w_0 - w_1||_1 up to that evaluation's rounding -- the test computes the
    minimum with the same predict, so the comparison is exact -- and the trace of loss_best never increases and never goes below
    it."""
    W = np.array([[0.9, 0.1], [0.7, 0.2], [1.5, 0.25], [0.6, 0.35]], dtype=np.float32)
    d = (W[:, 0] - W[:, 1]).astype(np.float64)
    assert (d > 0).all()
    x0 = np.array([[0.5, 0.25, 1.0, 0.75]], dtype=np.float32)
    eps = 0.125
    predict = lambda x: (np.asarray(x, dtype=np.float32) @ W).astype(np.float32)
    const = lambda it, max_iter, p_init: p_init
    r = R.run(predict, x0, [0], eps, 40, p_init=1.0, seed=3, schedule=const)
    z_min = predict(x0 - np.float32(eps))
    floor = np.float32(z_min[0, 0] - z_min[0, 1])
    analytic = float(x0[0].astype(np.float64) @ d) - eps * np.abs(d).sum()
    assert abs(float(floor) - analytic) <= 4 * np.spacing(np.float32(np.abs(predict(x0)).max()))  # fp32 evaluation of the analytic minimum
    signs = [R.draw(3, 0, 0, it, 1, 4, None, 1, 4, R.p_q(1.0)) for it in range(1, 40)]
    assert all(w == (0, 0, 1, 4) for w, _ in signs)
    first_minus = next(i for i, (_, m) in enumerate(signs, start=1) if m)  # the proposal, evaluated by query first_minus + 1
    trace = r["trace"][:, 0]
    assert r["losses"][first_minus, 0] == floor and trace[first_minus] == floor
    assert (np.diff(trace) <= 0).all() and (trace >= floor).all() and trace[-1] == floor
    assert same(r["x_best"], x0 - np.float32(eps)) and r["done"][0] == 0  # the margin stays positive: never done
    # the library's host twins walk the same path
    st = host_state(x0, 1, 4, 0, 3, eps)
    for it in range(40):
        host_step(st, predict(st["x_cand"]), np.zeros(1, dtype=np.int32), x0, 1, 4, 1, 4, R.p_q(1.0), 0, it, 3, eps, last=it == 39)
        assert st["loss_best"][0] == trace[it]
    assert same(st["x_best"], r["x_best"])
