"""The input-transformation defences without a GPU: the restatement of tests/defence_ref.py against NumPy's own median, convolution
and the quantiser's formula, lipasr.defences.lowpass_taps against the Hamming window's figures, the backward pass against inner
products and exact finite differences, the host twins (lipasr_defence_apply_host / lipasr_defence_vjp_host, the CPU-side handle on
the ABI) against the float32 restatement bit for bit at the shapes the GPU tests run, every refusal the launch functions make
before they touch a device, and the detector's arithmetic on given scores."""
import ctypes as C

import numpy as np
import pytest

import defence_ref as DR
from defence_ref import CASES, ids

import lipasr._native as N
from lipasr import defences as D


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def lengths_of(clips, n):
    return [None, DR.mixed_lengths(clips, n)]


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("k", [3, 5, 15])
def test_median_is_numpys_over_zero_padded_windows(k):
    x, _ = DR.inputs(3, 61)
    for nv in lengths_of(3, 61):
        nvc = DR.clamp_lengths(nv, 3, 61)
        out = DR.apply(x, [("median", k)], nv)
        for b in range(3):
            row = np.zeros(61 + k - 1)
            row[k // 2:k // 2 + nvc[b]] = x[b, :nvc[b]]
            want = np.median(np.lib.stride_tricks.sliding_window_view(row, k), axis=1)  # odd widths: nothing is averaged
            want[nvc[b]:] = 0
            assert np.array_equal(out[b], want), (k, nv, b)


@pytest.mark.parametrize("taps", [1, 9, 101, 255])
def test_fir_is_a_centred_convolution(taps):
    x, _ = DR.inputs(3, 300)
    h = DR.taps_for(taps)
    for nv in lengths_of(3, 300):
        nvc = DR.clamp_lengths(nv, 3, 300)
        out = DR.apply(x, [("fir", h)], nv)
        for b in range(3):
            want = np.zeros(300)
            if nvc[b]:
                full = np.convolve(x[b, :nvc[b]].astype(np.float64), h.astype(np.float64))  # "same" cut by hand: it would cut about
                want[:nvc[b]] = full[(taps - 1) // 2:(taps - 1) // 2 + nvc[b]]              # the longer operand when taps > nv
                if taps <= nvc[b]:
                    assert np.array_equal(want[:nvc[b]], np.convolve(x[b, :nvc[b]].astype(np.float64), h.astype(np.float64), "same"))
            assert np.abs(out[b] - want).max() <= 1e-12 * taps, (taps, nv, b)


@pytest.mark.parametrize("bits", [2, 8, 16])
def test_quantiser_is_its_formula(bits):
    x, _ = DR.inputs(3, 200)
    x[0, :9] = [-1.0, 1.0, 0.0, -0.0, 0.5 / 2 ** (bits - 1), 1.5 / 2 ** (bits - 1), -0.5 / 2 ** (bits - 1), 3.0, -3.0]  # ties go to even
    q = 2.0 ** (bits - 1)
    want = np.clip(np.rint(x.astype(np.float64) * q), -q, q - 1) / q
    for dtype in (np.float64, np.float32):
        out = DR.apply(x, [("quantize", bits)], None, dtype=dtype)
        assert out.dtype == dtype and np.array_equal(out, want)  # exact in fp32
    assert out[0, 0] == -1.0 and out[0, 1] == (q - 1) / q and out[0, 4] == 0 and out[0, 5] == min(2, q - 1) / q and out[0, 7] == (q - 1) / q
    nv = DR.mixed_lengths(3, 200)
    assert np.array_equal(DR.apply(x, [("quantize", bits)], nv), np.where(np.arange(200)[None, :] < np.clip(nv, 0, 200)[:, None], want, 0))


@pytest.mark.parametrize("name", [c for c in DR.CHAINS if len(DR.CHAINS[c]) > 1])
def test_a_chain_is_its_stages_composed(name):
    stages = DR.stages_of(name)
    x, g = DR.inputs(3, 333)
    for nv in lengths_of(3, 333):
        for dtype in (np.float64, np.float32):
            u = x.astype(dtype)
            for st in stages:
                u = DR.apply(u, [st], nv, dtype=dtype)
            assert np.array_equal(DR.apply(x, stages, nv, dtype=dtype), u)
        # backward: the stages in reverse, each at the input the forward pass gave it
        us = [x]
        for st in stages[:-1]:
            us.append(DR.apply(us[-1], [st], nv, dtype=np.float32))
        gg = g
        for st, u in zip(stages[::-1], us[::-1]):
            gg = DR.vjp(u, gg, [st], nv, dtype=np.float32)
        assert same(DR.vjp(x, g, stages, nv, dtype=np.float32), gg)


def test_fma32_rounds_once():
    """a b + c = (1 + 2^-23) + 2^-24 - 2^-70 lies just below the middle of two floats.  Rounded to float64 first it IS the middle,
    and the tie then goes to the even neighbour above; one rounding goes down."""
    a, b, c = np.float32(2.0 ** -12 * (1 + 2.0 ** -23)), np.float32(2.0 ** -12 * (1 - 2.0 ** -23)), np.float32(1 + 2.0 ** -23)
    assert float(a) * float(b) == 2.0 ** -24 * (1 - 2.0 ** -46)
    assert np.float32(float(c) + float(a) * float(b)) == np.float32(1 + 2.0 ** -22)  # the double rounding
    assert DR.fma32(np.array([a, -a]), np.array([b, b]), np.array([c, -c])).tolist() == [float(c), -float(c)]
    # and where the float64 sum is exact nothing is touched: 1 + 2^-24 is a tie and goes to even
    assert DR.fma32(np.array([np.float32(2.0 ** -24)]), np.array([np.float32(1)]), np.array([np.float32(1)]))[0] == np.float32(1)
    assert DR.fma32(np.array([np.float32(2.0 ** -24)]), np.array([np.float32(1)]), np.array([c]))[0] == np.float32(1 + 2.0 ** -22)


# ------------------------------------------------------------------------------------------------- lowpass_taps
def _gain(h, f_hz, sr):
    k = np.arange(len(h))
    return abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f_hz / sr * k)))


@pytest.mark.parametrize("cutoff,taps", [(4000, 101), (3000, 255), (6000, 61)])
def test_lowpass_taps(cutoff, taps):
    sr = 22050
    h = D.lowpass_taps(cutoff, sr, taps)
    assert h.dtype == np.float32 and h.shape == (taps,) and np.array_equal(h, h[::-1])
    assert abs(h.astype(np.float64).sum() - 1.0) <= 2.0 ** -22 and abs(_gain(h, 0.0, sr) - 1.0) <= 2.0 ** -22
    # The Hamming window's stop band: its highest side lobe lies 42.7 dB below its main lobe (Harris 1978, table 1), and a
    # windowed-sinc filter's stop band sits lower still, at about -53 dB (Oppenheim and Schafer, table 7.2: the ripple is the
    # window's spectrum INTEGRATED across the band edge).  The window's own figure is the bound that needs no trust in the design.
    stop = 10.0 ** (-42.7 / 20.0)
    assert _gain(h, sr / 2, sr) < stop
    # the transition band is the window's main lobe, 8 pi / taps rad wide in all: half of it on either side of the cutoff
    edge = 2.0 * sr / taps
    assert _gain(h, max(cutoff - edge, 0.0), sr) > 1.0 - stop and _gain(h, min(cutoff + edge, sr / 2), sr) < stop
    assert D.lowpass_taps(cutoff, sr).shape == (101,)
    for bad in ((0, sr, 101), (sr, sr, 101), (4000, sr, 100), (4000, sr, 257), (4000, 0, 101)):
        with pytest.raises(ValueError):
            D.lowpass_taps(*bad)


def test_bandpass_taps():
    sr = 22050
    h = D.bandpass_taps(300, 4000, sr, 255)
    assert h.dtype == np.float32 and np.array_equal(h, h[::-1])
    stop = 10.0 ** (-42.7 / 20.0)
    assert _gain(h, 0.0, sr) <= 2.0 ** -21 and _gain(h, sr / 2, sr) < stop and abs(_gain(h, 2000.0, sr) - 1.0) < 2 * stop
    with pytest.raises(ValueError):
        D.bandpass_taps(4000, 300, sr)


def test_parse_defence():
    st = D.parse_defence("median:5,lowpass:4000:101,quantize:8", 22050)
    assert [s[0] for s in st] == ["median", "lowpass", "quantize"] and st[0][1] == 5 and st[2][1] == 8
    assert same(st[1][1], D.lowpass_taps(4000, 22050, 101))
    assert same(D.parse_defence("bandpass:300:4000:61", 16000)[0][1], D.bandpass_taps(300, 4000, 16000, 61))
    assert D.parse_defence("lowpass:3000", 22050)[0][1].shape == (101,)
    chain, halo = D.chain_of(st)
    assert halo == 2 + 50 and [c[:2] for c in chain] == [(N.DEFENCE_MEDIAN, 5), (N.DEFENCE_FIR, 101), (N.DEFENCE_QUANTIZE, 8)]
    for bad in ("", "median", "median:x", "mp3:64", "lowpass:4000:100", "quantize:8:1"):
        with pytest.raises(ValueError):
            D.parse_defence(bad, 22050)
    for bad in ([], [("median", 5)] * 5, [("median", 4)], [("median", 17)], [("quantize", 1)], [("quantize", 17)], [("fir", np.zeros(4))],
                [("fir", np.zeros(257))], [("fir", np.zeros((3, 3)))], [("resample", 2)], [("fir", np.zeros(255))] * 3, ["median"]):
        with pytest.raises(ValueError):
            D.chain_of(bad)


# ------------------------------------------------------------------------------------------------- the backward pass
@pytest.mark.parametrize("name", ["fir31", "fir101-fir9", "fir255-fir255"])
def test_fir_chains_have_their_exact_adjoint(name):
    stages = [("fir", DR.taps_for(int(t[3:]), i)) for i, t in enumerate(name.split("-"))]
    x, g = DR.inputs(3, 700)
    for nv in lengths_of(3, 700):
        out, gx = DR.apply(x, stages, nv), DR.vjp(x, g, stages, nv)
        terms = np.abs(out * g).sum() + np.abs(x * gx).sum()
        assert abs((out * g).sum() - (x * gx).sum()) <= 1e-12 * terms, (name, nv)
        assert not gx[np.arange(700)[None, :] >= DR.clamp_lengths(nv, 3, 700)[:, None]].any()


@pytest.mark.parametrize("name", ["median3", "median15", "median5-fir", "median7-median3", "median3-median5-fir-fir"])
def test_median_routing_is_the_exact_finite_difference(name):
    """Inputs on a dyadic grid whose values differ from each other and from 0 by 2^-6 >= 4 delta, taps that are small dyadic numbers:
    every float64 operation is exact, no perturbation by delta changes an order (the medians come first in the chain: behind a FIR
    the values are sums, and nothing keeps those apart), and apply(x + delta e_s) - apply(x) is delta times
    column s of the routing matrix whose rows are vjp(x, e_t)."""
    n, delta = 29, 2.0 ** -10
    rng = np.random.default_rng(5)
    fir = lambda i: ("fir", (rng.integers(-8, 9, 5 + 2 * i) / 16.0).astype(np.float32))
    stages = [("median", int(t[6:])) if t.startswith("median") else fir(i) for i, t in enumerate(name.split("-"))]
    vals = np.concatenate([np.arange(1, 41), -np.arange(1, 41)]) * 2.0 ** -6
    x = np.stack([rng.permutation(vals)[:n] for _ in range(2)])
    for nv in (None, np.array([n, 17], dtype=np.int32)):
        base = DR.apply(x, stages, nv)
        eye = np.eye(n)
        routing = np.stack([DR.vjp(x, np.stack([eye[t]] * 2), stages, nv) for t in range(n)], axis=1)  # [clip][t][s]
        for s in range(n):
            xs = x.copy()
            xs[:, s] += delta
            assert np.array_equal(DR.apply(xs, stages, nv) - base, delta * routing[:, :, s]), (name, nv, s)
        if name.startswith("median") and "-" not in name:  # a median alone: every row routes to one in-clip element or to none
            assert set(np.unique(routing)) <= {0.0, 1.0} and (routing.sum(axis=2) <= 1).all()


def test_quantiser_gradient_is_straight_through_where_idle():
    x, g = DR.inputs(3, 200)  # U(-1.2, 1.2): both rails are met
    x[0, :4] = [1.0, -1.0, 127.4 / 128, -128.5 / 128]  # 1.0 -> rint 128 > q - 1: clamped; -1.0 -> -128: idle; 127.4 -> 127: idle
    q = 128.0
    r = np.rint(x.astype(np.float64) * q)
    idle = (r >= -q) & (r <= q - 1)
    assert idle[0, :4].tolist() == [False, True, True, True] and 0 < idle.mean() < 1  # -128.5 -> -128 (even): idle
    for dtype in (np.float64, np.float32):
        assert np.array_equal(DR.vjp(x, g, [("quantize", 8)], None, dtype=dtype), np.where(idle, g, 0))
    nv = DR.mixed_lengths(3, 200)
    inside = np.arange(200)[None, :] < np.clip(nv, 0, 200)[:, None]
    assert same(DR.vjp(x, g, [("quantize", 8)], nv, dtype=np.float32), np.where(idle & inside, g, np.float32(0)))
    assert same(N.defence_vjp_host(x, g, [(N.DEFENCE_QUANTIZE, 8, None)], n_valid=nv), np.where(idle & inside, g, np.float32(0)))


# ------------------------------------------------------------------------------------------------- the host twins
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_host_twins_equal_the_float32_restatement(case):
    name, clips, n = case
    stages = DR.stages_of(name)
    nat = DR.native(stages)
    for levels in (False, True):
        x, g = DR.inputs(clips, n, levels=levels)
        for nv in lengths_of(clips, n):
            out = N.defence_apply_host(x, nat, n_valid=nv, out=np.full((clips, n), np.nan, dtype=np.float32))
            assert same(out, DR.apply(x, stages, nv, dtype=np.float32)), (case, levels, nv)
            gx = N.defence_vjp_host(x, g, nat, n_valid=nv, out=np.full((clips, n), np.nan, dtype=np.float32))
            assert same(gx, DR.vjp(x, g, stages, nv, dtype=np.float32)), (case, levels, nv)


@pytest.mark.parametrize("taps", [31, 101, 255])
def test_fir_twin_is_as_close_to_float64_as_the_restatement(taps):
    """The repository's rule: the twin's worst error against the float64 restatement is within 8 x the float32 restatement's own."""
    x, g = DR.inputs(3, 2051)
    st = [("fir", DR.taps_for(taps))]
    for fn, twin in ((lambda dt: DR.apply(x, st, None, dtype=dt), N.defence_apply_host(x, DR.native(st))),
                     (lambda dt: DR.vjp(x, g, st, None, dtype=dt), N.defence_vjp_host(x, g, DR.native(st)))):
        truth = fn(np.float64)
        own = np.abs(fn(np.float32) - truth).max()
        assert own > 0 and np.abs(twin - truth).max() <= 8 * own


def test_ties_follow_the_position():
    """-0 and +0 tie; the earlier position wins the lower rank, so the selected element's bits and the routing say which one it was."""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    x = np.array([[nz, pz, nz, 1.0, -1.0, pz, nz]], dtype=np.float32)
    med = [(N.DEFENCE_MEDIAN, 3, None)]
    out = N.defence_apply_host(x, med)
    # t = 0: window (pad 0, -0, +0): all tie, rank 1 is position 0 -> -0.  t = 1: (-0, +0, -0) -> position 1, +0.  t = 2: (+0, -0, 1)
    # -> rank 1 is position 2 (-0).  t = 5: (-1, +0, -0) -> position 5 (+0).  t = 6: (+0, -0, pad 0) -> position 6, -0
    assert same(out, DR.apply(x, [("median", 3)], None, dtype=np.float32))
    assert np.signbit(out[0]).tolist() == [True, False, True, True, False, False, True]
    g = np.arange(1, 8, dtype=np.float32)[None, :]
    gx = N.defence_vjp_host(x, g, med)
    # t = 3: (-0, 1, -1) -> rank 1 is the -0 at position 2;  t = 4: (1, -1, +0) -> +0 at position 5
    assert gx[0].tolist() == [1.0, 2.0, 3.0 + 4.0, 0.0, 0.0, 5.0 + 6.0, 7.0]
    # a padding zero can be selected: its gradient is dropped
    x2 = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    assert N.defence_apply_host(x2, med)[0].tolist() == [1.0, 2.0, 2.0]
    assert N.defence_vjp_host(x2, np.ones((1, 3), dtype=np.float32), med)[0].tolist() == [1.0, 2.0, 0.0]
    x3 = np.array([[-1.0, 2.0, -3.0]], dtype=np.float32)  # t = 0: (pad, -1, 2) -> the pad; t = 2: (2, -3, pad) -> the pad
    assert N.defence_apply_host(x3, med)[0].tolist() == [0.0, -1.0, 0.0]
    assert N.defence_vjp_host(x3, np.ones((1, 3), dtype=np.float32), med)[0].tolist() == [1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------- the ABI
def test_abi_has_the_defences():
    names = ["lipasr_defence_apply", "lipasr_defence_vjp", "lipasr_defence_apply_host", "lipasr_defence_vjp_host",
             "lipasr_debug_defence_launches"]
    assert N.lib.lipasr_version() >= 740
    assert all(N.has(k) and hasattr(N.lib, k) and N.SINCE[k] == 740 and k in N.PROTOTYPES for k in names)
    assert N.lib.lipasr_debug_defence_launches(0) >= 0 and N.lib.lipasr_debug_defence_launches(1) >= 0
    assert N.lib.lipasr_debug_defence_launches(2) == -1 and N.lib.lipasr_debug_defence_launches(-1) == -1
    assert (N.DEFENCE_MAX_STAGES, N.DEFENCE_MAX_HALO) == (4, 256)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_launch_functions_refuse_before_the_device():
    """Every check of lipasr_defence_apply / lipasr_defence_vjp comes before the launch, so it is reached without a GPU; the
    pointers are host arrays that a refused call never reads, and a launch would fail on them."""
    x, g, out = (np.zeros((2, 8), dtype=np.float32) for _ in range(3))
    h = np.zeros(255, dtype=np.float32)
    before = [N.lib.lipasr_debug_defence_launches(k) for k in (0, 1)]

    def chain(stages):
        return N.defence_chain([(k, a) for k, a, _ in stages], [None if t is None else t.ctypes.data for _, _, t in stages])

    ap = lambda st, x_=_p(x), o=_p(out), clips=2, n=8: N.lib.lipasr_defence_apply(x_, None, *chain(st), clips, n, o, None)
    vj = lambda st, x_=_p(x), o=_p(out), clips=2, n=8, g_=_p(g): N.lib.lipasr_defence_vjp(x_, g_, None, *chain(st), clips, n, o, None)
    med, fir, qnt = (N.DEFENCE_MEDIAN, 5, None), (N.DEFENCE_FIR, 255, h), (N.DEFENCE_QUANTIZE, 8, None)
    for fn in (ap, vj):
        # the chain is checked first, also where there is nothing to do
        for kw in ({}, {"clips": 0}, {"n": 0}):
            assert fn([], **kw) == N.EINVAL and "stages" in N.last_error()
            assert fn([med] * 5, **kw) == N.EINVAL and "stages" in N.last_error()
            for k in (1, 2, 4, 17, -3):
                assert fn([(N.DEFENCE_MEDIAN, k, None)], **kw) == N.EINVAL and "median" in N.last_error()
            for k in (0, 2, 254, 257, -1):
                assert fn([(N.DEFENCE_FIR, k, h)], **kw) == N.EINVAL and "taps" in N.last_error()
            for k in (1, 17, 0, -8):
                assert fn([(N.DEFENCE_QUANTIZE, k, None)], **kw) == N.EINVAL and "bits" in N.last_error()
            assert fn([(3, 5, None)], **kw) == N.EINVAL and "kind" in N.last_error()
            assert fn([(N.DEFENCE_FIR, 255, None)], **kw) == N.EINVAL and "null" in N.last_error()
            assert fn([fir, fir, med, med]) == N.EINVAL and "halo" in N.last_error()  # 127 + 127 + 2 + 2 = 258
        assert fn([med], clips=-1) == N.EINVAL and fn([med], n=-8) == N.EINVAL
        # nothing to do: LIPASR_OK without a launch, whatever the pointers
        assert fn([med, fir, qnt], x_=None, o=None, clips=0) == N.OK and fn([fir, fir, (N.DEFENCE_MEDIAN, 5, None)], x_=None, o=None, n=0) == N.OK
        assert fn([med], x_=None) == N.EINVAL and "null" in N.last_error()
        assert fn([med], o=None) == N.EINVAL and "null" in N.last_error()
    assert vj([med], g_=None) == N.EINVAL and "null" in N.last_error()
    kinds, args, taps, count = chain([med])
    assert N.lib.lipasr_defence_apply(_p(x), None, None, args, taps, count, 2, 8, _p(out), None) == N.EINVAL
    assert N.lib.lipasr_defence_apply(_p(x), None, kinds, None, taps, count, 2, 8, _p(out), None) == N.EINVAL
    # an output that overlaps an input or the taps
    flat = np.zeros(400, dtype=np.float32)
    at = lambda off: C.c_void_p(flat.ctypes.data + 4 * off)
    assert ap([med], x_=at(0), o=at(15)) == N.EINVAL and "overlaps" in N.last_error()     # x [0, 16), out [15, 31)
    assert vj([med], x_=at(0), g_=at(40), o=at(50)) == N.EINVAL and "overlaps" in N.last_error()   # g [40, 56), gx [50, 66)
    k2, a2, _, c2 = chain([(N.DEFENCE_FIR, 255, h)])
    t2 = N.ptr_array([flat.ctypes.data + 4 * 100])
    assert N.lib.lipasr_defence_apply(at(0), None, k2, a2, t2, c2, 2, 8, at(350), None) == N.EINVAL and "taps" in N.last_error()  # taps [100, 355)
    # the host twins make the same checks
    assert N.lib.lipasr_defence_apply_host(at(0), None, *chain([med]), 2, 8, at(15)) == N.EINVAL
    assert N.lib.lipasr_defence_vjp_host(_p(x), _p(g), None, *chain([fir, fir, med, med]), 2, 8, _p(out)) == N.EINVAL and "halo" in N.last_error()
    with pytest.raises(ValueError):
        N.defence_apply_host(x, [(N.DEFENCE_MEDIAN, 4, None)])
    assert [N.lib.lipasr_debug_defence_launches(k) for k in (0, 1)] == before  # nothing was launched


def test_the_surface():
    from lipasr import attacks, estimators

    assert attacks.DefendedClassifier is estimators.DefendedClassifier
    assert issubclass(estimators.DefendedClassifier, estimators.WaveformClassifier)
    assert "DefendedClassifier" in estimators.__doc__ and "backward" in estimators.DefendedClassifier.__doc__
    with pytest.raises(TypeError):
        estimators.DefendedClassifier(object(), None)
    with pytest.raises(TypeError):
        D.TransformationDetector(object(), [])


# ------------------------------------------------------------------------------------------------- the detector's arithmetic
class _Base:
    predict_device = None


def test_detector_threshold_flags_and_auc():
    clean = np.array([0.30, 0.10, 0.20, 0.40, 0.00], dtype=np.float32)
    assert D.quantile_threshold(clean, 0.0) == pytest.approx(0.40) and D.quantile_threshold(clean, 1.0) == 0.0
    assert D.quantile_threshold(clean, 0.25) == pytest.approx(0.30) and D.quantile_threshold(clean, 0.125) == pytest.approx(0.35)
    big = np.random.default_rng(0).uniform(0, 1, 1000)
    thr = D.quantile_threshold(big, 0.05)
    assert thr == np.quantile(big, 0.95) and (big > thr).mean() == 0.05  # the clean false-positive rate is what was asked for
    det = D.TransformationDetector.__new__(D.TransformationDetector)
    det.threshold = None
    with pytest.raises(RuntimeError):
        det.flag_scores(clean)
    assert det.fit_scores(clean, 0.25) is det and det.threshold == pytest.approx(0.30)
    assert det.flag_scores(np.array([0.0, 0.30, 0.31, 2.0], dtype=np.float32)).tolist() == [False, False, True, True]
    for bad in (([], 0.05), (clean, -0.1), (clean, 1.5)):
        with pytest.raises(ValueError):
            D.quantile_threshold(*bad)
    a, b = np.array([0.1, 0.2, 0.3]), np.array([0.4, 0.5, 0.6, 0.9])
    assert D.roc_auc(a, b) == 1.0 and D.roc_auc(b, a) == 0.0 and D.roc_auc(a, a) == 0.5 and D.roc_auc(b, b.copy()) == 0.5
    assert D.roc_auc([0.0, 1.0], [0.5]) == 0.5 and D.roc_auc([0.0, 1.0, 2.0, 3.0], [2.5, 0.5]) == 0.5
    assert D.roc_auc([1, 2, 3, 4], [2, 5]) == (1 + 0.5 + 4) / 8
    assert D.TransformationDetector.roc_auc(a, b) == 1.0
    with pytest.raises(ValueError):
        D.roc_auc([], b)
