"""Local Lipschitz read-out on the MI355X: lipasr_jacobian_sigma against a float64 SVD of the same array, lipasr_mlp_jacobian
against the float64 oracle, and the read-outs built on them (get_local_lipschitz over features and over audio, lipschitz_report).

Bounds.  Kernel: 1e-5 -- the algorithm's own error is ~1e-8 (tests/test_local_lipschitz_cpu.py) and a dropped or doubled column
moves sigma^2 by order 1 / n >= 4.5e-5.  Classifier Jacobian: 2e-5 max |J|, the tolerance of test_class_gradient_and_output_vjp.
Audio: 8 x the error of the same oracle graph evaluated in float32 on the CPU, the factor of the backward-pass tests (2^-21 per
product in the forward kernels over fp32's 2^-24); the measured figures are in DESIGN.md ("Local Lipschitz read-out")."""
import wave

import numpy as np
import pytest
import torch

import local_lip_ref as R
import mfcc_grad_ref as G
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu


# =================================================================================================
# 1. the kernel against a float64 SVD of the same array
# =================================================================================================
def _place(J, layout, offset=0):
    """float32 [B, C, n] -> a device view [B, C, n] over [B][C][n] ("bcn") or class-major [C][B][n] ("cbn") storage that starts
    ``offset`` floats into its allocation."""
    B, C, n = J.shape
    buf = torch.zeros(B * C * n + offset, device="cuda")
    if layout == "bcn":
        view = buf[offset:].view(B, C, n)
    else:
        view = buf[offset:].view(C, B, n).permute(1, 0, 2)
    view.copy_(torch.as_tensor(J))
    return view


def _sigma(J, layout="bcn", offset=0):
    from lipasr.extract_features_construct_dataset import jacobian_sigma

    view = _place(np.asarray(J, dtype=np.float32), layout, offset)
    s, u, v = jacobian_sigma(view, return_vectors=True)
    s_only = jacobian_sigma(view)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(s.cpu().numpy(), s_only.cpu().numpy())  # (NaN compares equal to NaN here)
    return s.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()


def _check_against_svd(J, s, u, v, what, vectors=True):
    J64 = np.asarray(J, dtype=np.float32).astype(np.float64)
    for b in range(J64.shape[0]):
        want = R.sigma_uv(J64[b])[0]
        sb, ub, vb = float(s[b]), u[b].astype(np.float64), v[b].astype(np.float64)
        res = np.linalg.norm(J64[b].T @ (J64[b] @ vb) - sb * sb * vb)
        print(f"{what} sample {b}: sigma {sb:.8e} svd {want:.8e} rel {abs(sb - want) / want:.2e} | |u|-1 {abs(np.linalg.norm(ub) - 1):.2e} "
              f"|v|-1 {abs(np.linalg.norm(vb) - 1):.2e} residual / sigma^2 {res / want ** 2:.2e}")
        assert abs(sb - want) <= 1e-5 * want
        assert abs(np.linalg.norm(ub) - 1) <= 1e-5 and abs(np.linalg.norm(vb) - 1) <= 1e-5
        assert res <= 1e-5 * want ** 2
        if vectors:
            assert ub[np.argmax(np.abs(ub))] > 0
            assert np.linalg.norm(J64[b] @ vb - sb * ub) <= 2e-5 * want


def _random_jac(B, C, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, C, n)) * rng.uniform(0.2, 2.0, (B, C, 1))).astype(np.float32)


# the issue's shapes, then more class counts on either side of the kernel's row blocks (12, 20, block pairs above), each with
# 16-byte and with 4-byte loads
SHAPES = [(1, 10, 880), (3, 20, 2020), (2, 10, 22050), (5, 2, 1), (4, 32, 67), (3, 1, 130), (2, 10, 881),
          (2, 7, 36), (2, 6, 50), (2, 15, 260), (2, 14, 77), (2, 18, 131), (2, 27, 132), (2, 3, 1028)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", ["bcn", "cbn"])
def test_sigma_kernel_matches_svd(cuda, shape, layout):
    J = _random_jac(*shape, seed=sum(shape))
    _check_against_svd(J, *_sigma(J, layout), f"{shape} {layout}")


def test_sigma_kernel_declines_vector_loads_on_an_odd_base(cuda):
    J = _random_jac(3, 20, 2020, seed=5)
    a = _sigma(J, "bcn")
    for layout in ("bcn", "cbn"):
        b = _sigma(J, layout, offset=1)
        _check_against_svd(J, *b, f"offset 1 {layout}")
        np.testing.assert_allclose(b[0], a[0], rtol=2e-6)


# =================================================================================================
# 2. edges of the kernel
# =================================================================================================
@pytest.mark.parametrize("n", [881, 22050])
def test_single_entry(cuda, n):
    for col in (0, n - 1):
        J = np.zeros((2, 10, n), dtype=np.float32)
        J[0, 4, col] = 3.0
        J[1, 9, col] = -3.0
        s, u, v = _sigma(J)
        assert s[0] == 3.0 and s[1] == 3.0
        for b, (c, sign) in enumerate(((4, 1.0), (9, -1.0))):
            eu, ev = np.zeros(10, dtype=np.float32), np.zeros(n, dtype=np.float32)
            eu[c], ev[col] = 1.0, sign
            np.testing.assert_array_equal(u[b], eu)
            np.testing.assert_array_equal(v[b], ev)


def test_zero_rank_one_and_tied(cuda):
    rng = np.random.default_rng(8)
    s, u, v = _sigma(np.zeros((2, 10, 880), dtype=np.float32))
    assert not s.any() and not u.any() and not v.any()
    assert np.isfinite(s).all() and np.isfinite(u).all() and np.isfinite(v).all()
    # rank one
    a, b = rng.standard_normal(10), rng.standard_normal(881)
    J = np.outer(a, b).astype(np.float32)[None]
    s, u, v = _sigma(J)
    _check_against_svd(J, s, u, v, "rank one")
    ua = a / np.linalg.norm(a) * np.sign(a[np.argmax(np.abs(a))])
    assert np.abs(u[0] - ua).max() <= 1e-5
    assert abs(s[0] - np.linalg.norm(a) * np.linalg.norm(b)) <= 1e-5 * s[0]
    # two orthogonal rows of equal norm: any unit pair with J v = sigma u will do
    J = np.zeros((1, 2, 130), dtype=np.float32)
    J[0, 0, :65] = 1.5
    J[0, 1, 65:] = 1.5
    s, u, v = _sigma(J)
    _check_against_svd(J, s, u, v, "tied", vectors=False)


def test_power_of_two_scaling(cuda):
    J = _random_jac(2, 10, 880, seed=21)
    s0, u0, v0 = _sigma(J)
    for k in (-60, 40):
        s, u, v = _sigma(np.ldexp(J, k))
        rel = np.abs(s.astype(np.float64) - np.ldexp(s0.astype(np.float64), k)) / np.ldexp(s0.astype(np.float64), k)
        print(f"J 2^{k}: sigma relative deviation {rel.max():.2e}, u {np.abs(u - u0).max():.2e}, v {np.abs(v - v0).max():.2e}")
        assert rel.max() <= 1e-5 and np.abs(u - u0).max() <= 1e-5 and np.abs(v - v0).max() <= 1e-5
    # below what fp32 squares can hold: the ~1e-30 Jacobian of a saturated softmax
    s, u, v = _sigma((J.astype(np.float64) * 1e-30).astype(np.float32))
    _check_against_svd((J.astype(np.float64) * 1e-30).astype(np.float32), s, u, v, "1e-30")


def test_nan_stays_in_its_sample_and_runs_repeat(cuda):
    J = _random_jac(3, 10, 880, seed=22)
    a = _sigma(J)
    b = _sigma(J)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    for bad in (np.nan, np.inf):
        Jn = J.copy()
        Jn[1, 7, 501] = bad
        s, u, v = _sigma(Jn)
        assert np.isnan(s[1])
        for r in (0, 2):
            assert s[r] == a[0][r]
            np.testing.assert_array_equal(u[r], a[1][r])
            np.testing.assert_array_equal(v[r], a[2][r])


@pytest.mark.parametrize("layout", ["bcn", "cbn"])
def test_zero_columns_give_zero_v(cuda, layout):
    J = _random_jac(2, 10, 22050, seed=23)
    J[:, :, -1000:] = 0.0
    J[1, :, 300:340] = 0.0
    s, u, v = _sigma(J, layout)
    _check_against_svd(J, s, u, v, "zero tail")
    assert not v[:, -1000:].any() and not v[1, 300:340].any()
    assert (v[0, :-1000] != 0).all()


def test_sigma_argument_checks(cuda):
    from lipasr import _native as N
    from lipasr.extract_features_construct_dataset import jacobian_sigma

    with pytest.raises(ValueError):
        jacobian_sigma(torch.zeros(2, 33, 8, device="cuda"))
    with pytest.raises(ValueError):
        jacobian_sigma(torch.zeros(2, 8, device="cuda"))
    assert jacobian_sigma(torch.zeros(0, 10, 880, device="cuda")).shape == (0,)
    s, u, v = jacobian_sigma(torch.zeros(3, 10, 0, device="cuda"), return_vectors=True)
    assert not s.cpu().numpy().any() and not u.cpu().numpy().any() and v.shape == (3, 0)
    h = N.get_handle(0)
    assert N.lib.lipasr_jacobian_sigma(h.h, None, 0, 10, 880, 8800, 880, None, None, None, N.stream_ptr()) == N.OK


# =================================================================================================
# 3. lipasr_mlp_jacobian
# =================================================================================================
def _setup(spec, seed):
    p = R.setup_params(spec, seed)
    m = build_model(spec)
    load_params(m, p)
    return p, m


MLP_CASES = {"vd_37": (P.vd_constrained_spec, 37), "vd_1": (P.vd_constrained_spec, 1), "sr_5": (P.sr_constrained_spec, 5)}


@pytest.fixture(scope="module", params=sorted(MLP_CASES))
def mlp_case(request, cuda):
    from lipasr.attacks import TensorFlowV2Classifier

    make, batch = MLP_CASES[request.param]
    spec = make()
    p, m = _setup(spec, 7)
    n, C = spec[0].n_in, spec[-1].n_out
    x = np.random.default_rng(3).standard_normal((batch, n)).astype(np.float32)
    p64 = p.astype(np.float64)
    return dict(name=request.param, spec=spec, p=p, p64=p64, model=m, x=x, n=n, C=C,
                clf=TensorFlowV2Classifier(model=m, nb_classes=C, input_shape=(n,)),
                want={ol: R.jacobian(spec, p64, x, ol) for ol in (True, False)})


def _class_major(m, x, on_logits, probs=None):
    """lipasr_mlp_jacobian straight into [C][B][n] storage -> the [B, C, n] view."""
    from lipasr import _native as N

    b, n = x.shape
    c = m._n_classes
    jac = torch.zeros(c, b, n, device="cuda")
    N.check(N.lib.lipasr_mlp_jacobian(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(x), 1 if on_logits else 0, b, N.ptr(probs),
                                      N.ptr(jac), n, b * n, N.stream_ptr()))
    return jac.permute(1, 0, 2)


@pytest.mark.parametrize("on_logits", [True, False])
def test_mlp_jacobian_matches_the_oracle(mlp_case, on_logits):
    clf, x, C = mlp_case["clf"], dev(mlp_case["x"]), mlp_case["C"]
    want = mlp_case["want"][on_logits]
    scale = np.abs(want).max()
    probs = torch.empty(x.shape[0], C, device="cuda")
    got = clf.jacobian_device(x, on_logits=on_logits, probs_out=probs)
    assert got.shape == want.shape and got.is_contiguous()
    probs2 = torch.empty_like(probs)
    got_cm = _class_major(mlp_case["model"], x, on_logits, probs2)
    g, gc = got.cpu().numpy(), got_cm.cpu().numpy()
    print(f"{mlp_case['name']} on_logits {on_logits}: max |J| {scale:.3e}, worst error / max |J| {np.abs(g - want).max() / scale:.2e} "
          f"(class-major {np.abs(gc - want).max() / scale:.2e})")
    assert np.abs(g - want).max() <= 2e-5 * scale
    assert np.abs(gc - want).max() <= 2e-5 * scale
    np.testing.assert_array_equal(g, gc)  # the layout changes where a row is stored, not its bits
    for c in range(C):
        v = torch.zeros(x.shape[0], C, device="cuda")
        v[:, c] = 1.0
        row = clf.output_vjp_device(x, v, on_logits=on_logits).cpu().numpy()
        assert np.abs(g[:, c] - row).max() <= 2e-5 * scale
    if not on_logits:
        assert np.abs(g.sum(axis=1)).max() <= 1e-5 * scale  # probabilities sum to one: their gradients cancel
    pred = clf.predict(mlp_case["x"])
    np.testing.assert_array_equal(probs.cpu().numpy(), pred)
    np.testing.assert_array_equal(probs2.cpu().numpy(), pred)


def _gemm_launches():
    from lipasr import _native as N

    tot = 0
    for k in range(6):
        for xc in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    for ar in (0, 1, 2):
                        c = N.lib.lipasr_debug_gemm_launches(k, xc, a, b, ar, -1)
                        tot += c if c > 0 else 0
    return tot


def test_mlp_jacobian_launches_and_leaves_class_gradient_alone(mlp_case):
    clf, C, x = mlp_case["clf"], mlp_case["C"], mlp_case["x"]
    before = clf.class_gradient(x[:3])
    n0 = _gemm_launches()
    clf.jacobian_device(dev(x), on_logits=False)
    assert _gemm_launches() - n0 == len(mlp_case["spec"]) * (1 + C)  # one forward, C backward chains
    after = clf.class_gradient(x[:3])
    np.testing.assert_array_equal(before, after)


def test_mlp_jacobian_refuses_33_classes_and_bad_strides(cuda):
    from lipasr import _native as N
    from lipasr.attacks import TensorFlowV2Classifier

    # 33 classes are LIPASR_EINVAL (a ValueError here) -- already at lipasr_mlp_create, which makes no plan of more than 32
    # classes, so the Jacobian entry point's own check of its plan can never be the first to see one
    with pytest.raises(ValueError, match="33 classes"):
        spec = [P.LayerSpec(24, 16, True, 0.0, False), P.LayerSpec(16, 33, False, 0.0, False)]
        m = build_model(spec, max_batch=8)
        TensorFlowV2Classifier(model=m, nb_classes=33, input_shape=(24,)).jacobian_device(torch.zeros(4, 24, device="cuda"))
    x = torch.zeros(4, 24, device="cuda")
    jac = torch.zeros(4 * 32 * 24, device="cuda")
    spec = [P.LayerSpec(24, 16, True, 0.0, False), P.LayerSpec(16, 32, False, 0.0, False)]
    m = build_model(spec, max_batch=8)
    args = (m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(x), 1, 4, None, N.ptr(jac))
    assert N.lib.lipasr_mlp_jacobian(*args, 32 * 24, 24, N.stream_ptr()) == N.OK
    assert N.lib.lipasr_mlp_jacobian(*args, 24, 4 * 24, N.stream_ptr()) == N.OK
    for sb, sc in ((24, 24), (32 * 24, 23), (31 * 24, 24), (24, 3 * 24), (23, 4 * 24)):
        assert N.lib.lipasr_mlp_jacobian(*args, sb, sc, N.stream_ptr()) == N.EINVAL, (sb, sc)
    assert N.lib.lipasr_mlp_jacobian(*args[:5], 9, *args[6:], 32 * 24, 24, N.stream_ptr()) == N.EINVAL  # batch > max_batch
    torch.cuda.synchronize()


# =================================================================================================
# 4. the read-out over features
# =================================================================================================
def _product_bound(model):
    """prod_l ||W_l||_2 x prod_BN max_j |gamma_j| / sqrt(var_j + 1e-3), float64 on the host: a true upper bound of every sigma_b."""
    bound = 1.0
    for layer in model.layers:
        ws = [np.asarray(w, dtype=np.float64) for w in layer.get_weights()]
        if "dense" in layer.name:
            bound *= np.linalg.norm(ws[0], 2)
        elif "batch" in layer.name:
            bound *= np.max(np.abs(ws[0]) / np.sqrt(ws[3] + P.BN_EPS))
    return bound


def test_local_lipschitz_over_features(mlp_case):
    from lipasr.extract_features_construct_dataset import get_local_lipschitz

    clf, x = mlp_case["clf"], mlp_case["x"]
    want = R.sigmas(mlp_case["want"][True])
    got, u, v = get_local_lipschitz(clf, x, return_vectors=True)
    assert got.dtype == np.float64 and got.shape == (x.shape[0],) and u.shape == (x.shape[0], mlp_case["C"]) and v.shape == x.shape
    np.testing.assert_array_equal(got, get_local_lipschitz(clf, x))
    rel = np.abs(got - want) / want
    bound = _product_bound(mlp_case["model"])
    print(f"{mlp_case['name']}: local Lipschitz constants {got.min():.4f} .. {got.max():.4f}, worst relative error {rel.max():.2e}; "
          f"product bound {bound:.4e}")
    assert rel.max() <= 2e-5
    assert (got <= bound).all()
    for b in range(min(3, x.shape[0])):  # v is the direction the logits move fastest along
        J = mlp_case["want"][True][b]
        assert abs(np.linalg.norm(J @ v[b]) - want[b]) <= 2e-5 * want[b]
    # probabilities: another Jacobian, the same read-out
    gp = get_local_lipschitz(clf, x[:2], on_logits=False)
    wp = R.sigmas(mlp_case["want"][False][:2])
    assert (np.abs(gp - wp) <= 2e-5 * wp).all()


def test_local_lipschitz_chunks(cuda, monkeypatch):
    from lipasr import extract_features_construct_dataset as E
    from lipasr.attacks import TensorFlowV2Classifier

    spec = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
    p = R.setup_params(spec, 2)
    m = build_model(spec, max_batch=4)
    load_params(m, p)
    clf = TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,))
    x = np.random.default_rng(4).standard_normal((11, 36)).astype(np.float32)
    whole = E.get_local_lipschitz(clf, x)  # three chunks of the batch limit
    monkeypatch.setattr(E, "JACOBIAN_CHUNK_BYTES", 3 * 4 * 5 * 36)  # three rows per chunk
    np.testing.assert_array_equal(E.get_local_lipschitz(clf, x), whole)
    want = R.sigmas(R.jacobian(spec, p.astype(np.float64), x, True))
    assert (np.abs(whole - want) <= 2e-5 * want).all()
    assert E.get_local_lipschitz(clf, x[:0]).shape == (0,)


def test_lip_stats_callback_probe(cuda, capsys):
    from lipasr.extract_features_construct_dataset import get_local_lipschitz
    from lipasr.attacks import TensorFlowV2Classifier
    from lipasr.train_constraints import lip_stats_callback

    spec = P.vd_constrained_spec()
    _, m = _setup(spec, 5)
    probe = np.random.default_rng(6).standard_normal((4, 880)).astype(np.float32)
    cb = lip_stats_callback()
    cb.set_model(m)
    cb.on_epoch_begin(0)
    plain = capsys.readouterr().out
    assert "local Lipschitz" not in plain and "The Lipschitz constant on epoch 0 is" in plain
    cb = lip_stats_callback(probe=probe)
    cb.set_model(m)
    cb.on_epoch_begin(0)
    out = capsys.readouterr().out
    assert out.startswith(plain)
    want = get_local_lipschitz(TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,)), probe).max()
    assert f"The largest local Lipschitz constant over 4 probe rows on epoch 0 is {want}" in out


# =================================================================================================
# 5. the read-out over audio
# =================================================================================================
L = 44


def _mean_features(clips, kw):
    """The StandardScaler mean of the audio cases: the float64 oracle features of ``clips``, averaged (a mean taken from the one or
    two rows under test would put the standardised features, and with zero biases every pre-activation, at zero)."""
    with torch.no_grad():
        return np.stack([G.features(torch.as_tensor(c.astype(np.float64)), **kw).numpy() for c in clips]).mean(axis=0)


def _audio_rows(name, cuda):
    """-> (classifier, device rows, lengths or None, per row: (numpy row, n_clip), oracle keywords, spec, params)"""
    from lipasr.attacks import WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(11)
    if name == "short":
        from lipasr.speaker_recognition import waveform_classifier

        spec = P.sr_unconstrained_spec()
        p = R.setup_params(spec, 3)
        m = build_model(spec, max_batch=8)
        load_params(m, p)
        w = G.short_parity_clips(441, 220, 22050)[:1]
        kw = dict(n_fft=441, hop=220, utterance_length=101, domain="22k")
        mean, scale = _mean_features(G.short_parity_clips(441, 220, 22050), kw), rng.uniform(0.5, 2.0, 2020)
        clf = waveform_classifier(m, mean, scale, batch_max=4)
        return clf, torch.as_tensor(w).to(cuda), None, [(r, None) for r in w], kw, spec, p, mean, scale
    spec = P.vd_unconstrained_spec()
    p = R.setup_params(spec, 3)
    m = build_model(spec, max_batch=8)
    load_params(m, p)
    ex = MfccExtractor(16000, 16000, batch_max=4)
    domain = "input" if name.endswith("input") else "22k"
    clips16 = G.parity_clips(16000)
    if name.startswith("ragged"):
        w = np.zeros((2, 16000), dtype=np.float32)
        w[0, :12000] = G.parity_clips(12000)[2]
        w[1] = clips16[0]
        lens = np.array([12000, 16000], dtype=np.int32)
    elif name == "whole_22k":
        w, lens = clips16[[0, 2]], None
    else:
        w, lens = clips16[1:2], None
    wt = torch.as_tensor(w).to(cuda).contiguous()
    lt = None if lens is None else torch.as_tensor(lens).to(cuda)
    rows = ex.resample(wt, n_valid=lt) if domain == "22k" else wt
    rows_np = rows.cpu().numpy()
    ratio = 22050.0 / 16000.0
    clip = lambda n: int(np.ceil(n * ratio)) if domain == "22k" else int(n)
    per_row = [(rows_np[i], None if lens is None else clip(lens[i])) for i in range(len(w))]
    kw = dict(sr_in=16000, utterance_length=L, domain=domain)
    mean, scale = _mean_features(clips16, dict(sr_in=16000, utterance_length=L, domain="input")), rng.uniform(0.5, 2.0, 20 * L)
    clf = WaveformClassifier(m, 10, extractor=ex, utterance_length=L, mean=mean, scale=scale, domain=domain)
    return clf, rows, lt, per_row, kw, spec, p, mean, scale


AUDIO_CASES = ["whole_22k", "whole_input", "ragged_22k", "ragged_input", "short"]


@pytest.fixture(scope="module")
def audio(cuda):
    """Every audio case with its oracle, computed once: per row the float64 Jacobian and sigma and the errors of the SAME graph
    evaluated in float32 (the yardstick), and ``sigma_yard``, the worst float32 sigma error over ALL rows of ALL cases."""
    cases = {}
    for name in AUDIO_CASES:
        clf, rows, lt, per_row, kw, spec, p, mean, scale = _audio_rows(name, cuda)
        oracle = []
        for row, n_clip in per_row:
            J64 = R.audio_jacobian(spec, p.astype(np.float64), row, mean, scale, n_clip=n_clip, **kw)
            J32 = R.audio_jacobian(spec, p, row, mean, scale, dtype=torch.float32, n_clip=n_clip, **kw)
            s64, s32 = R.sigma_uv(J64)[0], R.sigma_uv(J32)[0]
            oracle.append(dict(J64=J64, s64=s64, s32=s32, n_clip=n_clip, y_s=abs(s32 - s64) / s64,
                               y_rows=[G.errs(J32[c], J64[c]) for c in range(J64.shape[0])]))
        cases[name] = dict(clf=clf, rows=rows, lt=lt, oracle=oracle)
    sigma_yard = max(o["y_s"] for c in cases.values() for o in c["oracle"])
    yield dict(cases=cases, sigma_yard=sigma_yard)
    for c in cases.values():
        c["clf"].extractor.close()


@pytest.mark.parametrize("name", AUDIO_CASES)
def test_local_lipschitz_over_audio(audio, cuda, name):
    """MI355X figures: DESIGN.md, "Local Lipschitz read-out".  Bounds: 8 x the float32 evaluation of the oracle.  Each class row is
    held to the worst row figure of its case, in its own norm.  sigma is held to 8 x the worst float32 sigma error over all rows of
    all five cases: that error is ONE number per row of audio, and a single one can vanish by luck (1.6e-9 on the 441/220 window,
    below the 6e-8 resolution of the float32 the device returns), so the worst of the seven stands for the figure."""
    from lipasr.extract_features_construct_dataset import get_local_lipschitz, jacobian_sigma

    case = audio["cases"][name]
    clf, rows, lt, oracle = case["clf"], case["rows"], case["lt"], case["oracle"]
    C, B = clf.nb_classes, rows.shape[0]
    jac = clf.jacobian_device(rows, on_logits=True, lengths=lt)
    assert tuple(jac.shape) == (B, C, clf.n)
    # every class row carries the bits of its own output_vjp_device call, which reruns the extraction
    for c in range(C):
        v = torch.zeros(B, C, device=cuda)
        v[:, c] = 1.0
        assert torch.equal(jac[:, c], clf.output_vjp_device(rows, v, on_logits=True, lengths=lt)), c
    keep = jac.clone()
    assert torch.equal(clf.jacobian_device(rows, on_logits=True, lengths=lt), keep)
    got = keep.double().cpu().numpy()
    assert np.isfinite(got).all()
    sig, u, v = get_local_lipschitz(clf, rows, lengths=lt, return_vectors=True)
    np.testing.assert_array_equal(sig, jacobian_sigma(keep).double().cpu().numpy())
    devs = []
    for b, o in enumerate(oracle):
        n_clip = o["n_clip"]
        if n_clip is not None:  # nothing past the clip's end: the Jacobian, and therefore v, is exactly zero there
            assert not got[b, :, n_clip:].any() and not v[b, n_clip:].any()
            assert np.abs(got[b, :, :n_clip]).max() > 0
        for c in range(C):
            devs.append((b, c) + G.errs(got[b, c], o["J64"][c]) + (abs(sig[b] - o["s64"]) / o["s64"],))
        print(f"audio {name} row {b}: sigma device {sig[b]:.6e} float64 {o['s64']:.6e} float32 oracle {o['s32']:.6e} (its error "
              f"{o['y_s']:.3e}); worst class row: device inf {max(d[2] for d in devs if d[0] == b):.3e} two "
              f"{max(d[3] for d in devs if d[0] == b):.3e}")
    y_inf, y_2 = (max(y[i] for o in oracle for y in o["y_rows"]) for i in range(2))
    y_s = audio["sigma_yard"]
    print(f"audio {name}: yardstick (worst float32 oracle) inf {y_inf:.3e} two {y_2:.3e} sigma over all cases {y_s:.3e}; worst device "
          f"inf {max(d[2] for d in devs):.3e} two {max(d[3] for d in devs):.3e} sigma {max(d[4] for d in devs):.3e}")
    for b, c, e_inf, e_2, e_s in devs:
        assert e_inf <= 8 * y_inf, (b, c, e_inf)
        assert e_2 <= 8 * y_2, (b, c, e_2)
        assert e_s <= 8 * y_s, (b, e_s)
    if name == "short":
        with pytest.raises(ValueError):
            clf.jacobian_device(rows, lengths=[22050])


def test_local_lipschitz_of_a_bare_estimator(cuda):
    """get_local_lipschitz asks its estimator for jacobian_device and nb_classes only; without a batch_limit it chunks by bytes."""
    from lipasr.attacks import TensorFlowV2Classifier
    from lipasr.extract_features_construct_dataset import get_local_lipschitz

    spec = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
    m = build_model(spec, max_batch=4)
    load_params(m, R.setup_params(spec, 2))
    clf = TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,))
    assert clf.batch_limit == 4

    class Bare:
        nb_classes = 5

        def jacobian_device(self, xt, on_logits=True):
            return clf.jacobian_device(xt, on_logits=on_logits)

    x = np.random.default_rng(4).standard_normal((11, 36)).astype(np.float32)
    np.testing.assert_array_equal(get_local_lipschitz(Bare(), x), get_local_lipschitz(clf, x))


def test_shared_surface_on_a_feature_estimator(cuda):
    """The device-side surface of lipasr.estimators on a TensorFlowV2Classifier: 7 rows through a model that takes 4 at a time.
    Every comparison is bit for bit -- the surface only routes to calls that existed before it."""
    from lipasr import _native as N
    from lipasr.attacks import TensorFlowV2Classifier

    spec = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
    m = build_model(spec, max_batch=4)
    load_params(m, R.setup_params(spec, 2))
    clf = TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,))
    assert clf.clip_values is None and clf.batch_limit == 4 and clf.input_shape == (36,) and clf.nb_classes == 5 and clf.model is m
    rng = np.random.default_rng(4)
    x_np = rng.standard_normal((7, 36)).astype(np.float32)
    y_np = G.onehot(rng.integers(0, 5, 7), 5).astype(np.float32)
    x, y = clf.rows_device(x_np), dev(y_np)
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (7, 36)
    with pytest.raises(ValueError):
        clf.rows_device(x_np[:, :35])
    assert torch.equal(clf.predict_device(x, logits=True), m.predict_device(x, logits=True))
    assert clf.lengths_device(None, 7) is None
    refusal = "lengths= is for attacks over audio: the estimator must be a WaveformClassifier"
    for call in (lambda: clf.predict_device(x, lengths=[36] * 7), lambda: clf.jacobian_device(x, lengths=[36] * 7),
                 lambda: clf.loss_gradient_device(x, y, lengths=[36] * 7), lambda: clf.lengths_device([36] * 7, 7)):
        with pytest.raises(ValueError, match=refusal):
            call()
    want = torch.empty(7, 5, device="cuda")
    for s in range(0, 7, 3):
        x0 = x[s:s + 3]
        N.check(N.lib.lipasr_mlp_own_labels(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(x0), x0.shape[0], N.ptr(want[s:s + 3]), N.stream_ptr()))
    assert torch.equal(clf.own_labels_device(x, batch=3), want)
    assert torch.equal(clf.own_labels_device(x, batch=64), clf.own_labels_device(x))  # never more than batch_limit rows a call
    assert bool((want.sum(dim=1) == 1).all()) and bool(((want == 0) | (want == 1)).all())
    g = clf.loss_gradient_device(x, y)
    assert g.cpu().numpy().tobytes() == clf.loss_gradient(x_np, y_np).tobytes() and float(g.abs().max()) > 0
    out = torch.empty_like(x)
    assert clf.loss_gradient_device(x, y, out=out) is out and torch.equal(out, g)


# =================================================================================================
# 6. lipschitz_report
# =================================================================================================
def test_lipschitz_report(cuda, tmp_path, capsys):
    from lipasr import attack_eval as V, attacks as A
    from lipasr.extract_features_construct_dataset import (compute_mfcc_all_files, get_lipschitz_constrained, get_local_lipschitz,
                                                           get_norms, get_upper_lipschitz)
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(24, seed=31)
    files = []
    for i in range(24):
        path = tmp_path / f"clip_{i:03d}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(waves[i], -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats = compute_mfcc_all_files(files)
    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=8)
    load_params(m, R.setup_params(spec, 3))
    models = {"constrained": m, "unconstrained": m}
    train, val, test = feats[:8], feats[8:16], feats[16:24]
    upper, cons = get_upper_lipschitz(get_norms(m)), get_lipschitz_constrained(m)
    capsys.readouterr()
    # over the MFCC rows
    rep = V.lipschitz_report(models, train, val, test, over="mfcc")
    out = capsys.readouterr().out
    x = A.standardize_dataset(train, val, test)[2]
    want = get_local_lipschitz(A.TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,)), x)
    for name in models:
        r = rep[name]
        np.testing.assert_array_equal(r["local"], want)
        assert (r["max"], r["mean"], r["median"]) == (want.max(), want.mean(), np.median(want))
        assert r["upper"] == upper and r["constrained"] == cons
    assert f"Upper Lipschitz bound: {upper}" in out and f"Upper Lipschitz bound unconstrained: {upper}" in out
    assert f"Lipschitz constant with the BatchNorm correction: {cons}" in out
    assert f"Local Lipschitz constant over 8 test rows: max {want.max()} mean {want.mean()} median {np.median(want)}" in out
    assert len(V.lipschitz_report(models, train, val, test, over="mfcc", limit=3)["constrained"]["local"]) == 3
    # over the audio of the files
    tr, va, _ = A.standardize_dataset(train, val, test)
    clean = A.black_box_attack_on_audio_dataset(files[16:24], 0, p=0, alpha=0)
    sc = A.StandardScaler().fit(np.concatenate([np.asarray(tr), np.asarray(va), clean]))
    capsys.readouterr()
    for domain in ("22k", "input"):
        rep = V.lipschitz_report(models, train, val, test, over="audio", test_filenames=files[16:24], domain=domain)
        out = capsys.readouterr().out
        ex = A._extractor(16000, 16000, 8)
        clf = A.WaveformClassifier(m, 10, extractor=ex, mean=sc.mean_, scale=sc.scale_, domain=domain)
        w = A._to_dev(np.stack([A.read_wav(f)[0] for f in files[16:24]]))
        want = get_local_lipschitz(clf, ex.resample(w) if domain == "22k" else w)
        assert want.shape == (8,) and (want > 0).all()
        for name in models:
            np.testing.assert_array_equal(rep[name]["local"], want)
            assert rep[name]["upper"] == upper and rep[name]["constrained"] == cons
        assert f"Local Lipschitz constant over 8 test files: max {want.max()} mean {want.mean()} median {np.median(want)}" in out
        assert f"Upper Lipschitz bound: {upper}" in out
    with pytest.raises(ValueError):
        V.lipschitz_report(models, train, val, test, over="audio")
    with pytest.raises(ValueError):
        V.lipschitz_report(models, train, val, test, over="mel")
