"""Bound propagation on the device: lipasr_mlp_bounds against the float64 restatement of tests/bounds_ref.py (the checks of
tests/bounds_checks.py: enclosure, tightness, sampling, agreement) at workspace offsets 0 and 1 float, against the host twin, and
twice for the same bits; launch counts on the reference shape; the Python surface of lipasr.bounds (certified_radius against the
float64 driver, monotone, under every PGD flip), get_robustness_radius, attack_eval's certify report and the refusal over audio.

Device and host twin: EQUAL VALUES everywhere (np.array_equal).  The design keeps the k order -- the MFMA is an fmaf chain in
ascending k, every other sum is a butterfly per 32 columns and then index order, which the host restates -- so nothing is left to
a tolerance; only the sign of a zero may differ (the padded k steps of the last tile turn a -0 accumulator into +0)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bounds_checks as K
import bounds_ref as R

import lipasr._native as N
import lipasr.keras as KS

pytestmark = pytest.mark.gpu

INF = float("inf")
CASES = R.cases()
NORMS = [INF, 2]
GRID = [(c, n) for c in CASES for n in NORMS]
IDS = [f"{c}-{'inf' if n == INF else 2}" for c, n in GRID]
REF_WIDTHS = [880, 1024, 512, 256, 128, 64, 10]


def build(m, max_batch=128):
    """The lipasr.keras.Model of a bounds_ref model, through the layer protocol."""
    KS.reset_layer_names()
    inp = KS.Input((m["widths"][0],))
    node = inp
    L = len(m["W"])
    for l in range(L):
        node = KS.Dense(m["widths"][l + 1], activation="softmax" if l + 1 == L else "relu")(node)
        if m["bn"][l] is not None:
            node = KS.BatchNormalization()(node)
    model = KS.Model(inputs=inp, outputs=node, max_batch=max_batch)
    model.compile(optimizer="adam", loss=KS.CategoricalCrossentropy(), metrics=["accuracy"])
    dense = [l for l in model.layers if "dense" in l.name]
    bns = {l._index: l for l in model.layers if "batch" in l.name}
    for l, layer in enumerate(dense):
        layer.set_weights([m["W"][l], m["b"][l]])
        if l in bns:
            bns[l].set_weights(list(m["bn"][l]))
    return model


@functools.lru_cache(maxsize=None)
def model_of(case):
    return build(CASES[case][0])


def estimator(model):
    from lipasr.attacks import TensorFlowV2Classifier

    return TensorFlowV2Classifier(model=model, nb_classes=model._n_classes, input_shape=(model._widths[0],))


def device_call(model, x, eps, y, norm, clip=R.CLIP, ws_offset=0, crown=True):
    """One lipasr_mlp_bounds with the workspace ``ws_offset`` floats into its allocation -> the dict of tests/bounds_checks.py."""
    b, w = x.shape[0], model._widths
    c = w[-1]
    need = C.c_size_t()
    N.check(N.lib.lipasr_mlp_bounds_workspace(model._plan, b, C.byref(need)))
    ws = torch.zeros(need.value + ws_offset, device="cuda")[ws_offset:]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dt).contiguous()
    xt, et, yt = t(x, torch.float32), t(eps, torch.float32), t(y, torch.int32)
    fam = b * (w[0] + 2 * sum(w[1:-1]))
    out = {"margin_ibp": torch.full((b, c), 7.0, device="cuda"), "margin_crown": torch.full((b, c), 7.0, device="cuda") if crown else None,
           "slack": torch.full((b, c), 7.0, device="cuda") if crown else None, "lo": torch.zeros(fam, device="cuda"),
           "hi": torch.zeros(fam, device="cuda")}
    N.check(N.lib.lipasr_mlp_bounds(model._plan, N.ptr(model._params), N.ptr(model._bnstate), N.ptr(xt), N.ptr(et), float(norm), clip[0], clip[1],
                                    N.ptr(yt), b, N.ptr(ws), need.value, N.ptr(out["margin_ibp"]), N.ptr(out["margin_crown"]), N.ptr(out["slack"]),
                                    N.ptr(out["lo"]), N.ptr(out["hi"]), N.stream_ptr()))
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def run(case, norm, ws_offset=0):
    m, B = CASES[case]
    x, eps, y = R.case_inputs(m, B, len(case))
    return device_call(model_of(case), x, eps, y, norm, ws_offset=ws_offset), m, x, eps, y


def host(case, norm):
    m, B = CASES[case]
    x, eps, y = R.case_inputs(m, B, len(case))
    params, state = R.pack(m, N.bounds_layout(m["widths"], R.bn_flags(m)))
    return N.mlp_bounds_host(m["widths"], R.bn_flags(m), params, state, x, eps, norm, y, clip_lo=R.CLIP[0], clip_hi=R.CLIP[1])


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize("ws_offset", [0, 1])
@pytest.mark.parametrize("case,norm", GRID, ids=IDS)
def test_device_against_float64(case, norm, ws_offset):
    out, m, x, eps, y = run(case, norm, ws_offset)
    worst = K.check_enclosure_and_tightness(out, m, x, eps, norm, R.CLIP)
    K.check_sampling(out, m, x, eps, norm, R.CLIP, y, seed=7)
    agree = K.check_agreement(out, m, x, eps, norm, R.CLIP, y)
    print(f"{case} norm {norm} offset {ws_offset}: loosest side {worst:.3f} w, margin_crown |difference| / bound {agree:.3f}")
    assert same_bits(out, run(case, norm, 0)[0])


@pytest.mark.parametrize("case,norm", GRID, ids=IDS)
def test_device_equals_host_twin(case, norm):
    dev, twin = run(case, norm)[0], host(case, norm)
    for k in dev:
        fin = np.isfinite(dev[k]) & np.isfinite(twin[k])
        print(f"{case} norm {norm} {k}: max |device - host| {np.abs(dev[k][fin].astype(np.float64) - twin[k][fin]).max():.3e}")
    for k in dev:
        assert np.array_equal(dev[k], twin[k]), k


@pytest.mark.parametrize("case", ["signed70", "wide"])
def test_two_calls_give_the_same_bits(case):
    m, B = CASES[case]
    x, eps, y = R.case_inputs(m, B, len(case))
    a = device_call(model_of(case), x, eps, y, INF)
    b = device_call(model_of(case), x, eps, y, INF)
    assert same_bits(a, b)


def test_known_answers_on_the_device():
    m, B = CASES["linear"]
    x, _, y = R.case_inputs(m, B, 0)
    eps = np.array([0.0, 0.05, 0.5], np.float32)
    W, b = m["W"][0].astype(np.float64), m["b"][0].astype(np.float64)
    for norm in NORMS:
        out = device_call(model_of("linear"), x, eps, y, norm, clip=(-INF, INF))
        for r in range(B):
            d = W[:, [y[r]]] - W
            want = x[r].astype(np.float64) @ d + b[y[r]] - b - float(eps[r]) * (np.abs(d).sum(0) if norm == INF else np.sqrt((d * d).sum(0)))
            k = np.arange(3) != y[r]
            tol = out["slack"][r] + np.abs(d).sum(0) * K.spacing32(np.abs(x[r]).max() + eps[r]) + K.spacing32(want)
            for name in ("margin_ibp", "margin_crown"):
                assert (np.abs(out[name][r] - want)[k] <= tol[k]).all() and (out[name][r][k] <= want[k]).all()
    # the two neurons of tests/test_bounds_cpu.py: CROWN 1.0, IBP -0.5
    hand = {"widths": [1, 2, 2], "W": [np.array([[1.0, 1.0]], np.float32), np.eye(2, dtype=np.float32)],
            "b": [np.array([0.5, 2.0], np.float32), np.zeros(2, np.float32)], "bn": [None, None]}
    out = device_call(build(hand), np.zeros((1, 1), np.float32), np.ones(1, np.float32), np.array([1], np.int32), INF, clip=(-INF, INF))
    sl = float(out["slack"][0, 0])
    assert 0 < sl < 1e-5 and 1.0 - 2 * sl - 1e-6 <= out["margin_crown"][0, 0] <= 1.0 and -0.5 - 1e-5 <= out["margin_ibp"][0, 0] <= -0.5


def test_a_nan_and_a_bad_row_stay_in_their_rows():
    m, B = CASES["signed70"]
    x, eps, y = R.case_inputs(m, B, len("signed70"))
    good = run("signed70", INF)[0]
    xb, eb, yb = x.copy(), eps.copy(), y.copy()
    xb[1, 5], eb[33], yb[69] = np.nan, -1.0, 5
    bad = device_call(model_of("signed70"), xb, eb, yb, INF)
    rows = np.array([1, 33, 69])
    keep = np.setdiff1d(np.arange(B), rows)
    for name in ("margin_ibp", "margin_crown", "slack"):
        assert np.isnan(bad[name][rows]).all() and np.array_equal(bad[name][keep], good[name][keep])


def test_launch_counts_on_the_reference_shape():
    m = R.make_model(REF_WIDTHS, 9, bn=(0, 1, 2, 3, 4), signed=False, scale=0.5)
    model = build(m, max_batch=8)
    x = np.random.default_rng(5).standard_normal((8, 880)).astype(np.float32)
    y = R.forward(m, x).argmax(-1).astype(np.int32)
    eps = np.full(8, 0.01, np.float32)
    count = lambda: [N.lib.lipasr_debug_bounds_launches(i) for i in range(5)]
    c0 = count()
    out = device_call(model, x, eps, y, INF, clip=(-INF, INF))
    c1 = count()
    device_call(model, x, eps, y, 2, clip=(-INF, INF), crown=False)
    c2 = count()
    L = len(REF_WIDTHS) - 1
    assert [b - a for a, b in zip(c0, c1)] == [1, L - 1, 1, L - 1, 1]  # forward L + 1, backward L
    assert [b - a for a, b in zip(c1, c2)] == [1, L - 1, 1, 0, 0]      # no backward pass without margin_crown
    K.check_enclosure_and_tightness(out, m, x, eps, INF, (-INF, INF))
    K.check_agreement(out, m, x, eps, INF, (-INF, INF), y)
    # the Python surface refuses audio: the estimator in front of this model is a WaveformClassifier
    from lipasr.attacks import WaveformClassifier
    from lipasr.bounds import bound_margins
    from lipasr.extract_features_construct_dataset import MfccExtractor

    ex = MfccExtractor(16000, 16000, batch_max=8)
    try:
        wc = WaveformClassifier(model, 10, extractor=ex, utterance_length=44, domain="22k")
        with pytest.raises(TypeError, match="MFCC stage's log has no interval form"):
            bound_margins(wc, np.zeros((1, 16000), np.float32), 0.01)
    finally:
        ex.close()


# ------------------------------------------------------------------------------------------------------- the Python surface
def _rows(n=32, seed=11):
    m = CASES["nonneg"][0]
    x = np.clip(np.random.default_rng(seed).standard_normal((n, 37)), -2.4, 2.4).astype(np.float32)
    return m, x, R.forward(m, x).argmax(-1).astype(np.int32)


def test_bound_margins_chunks_and_methods():
    from lipasr.bounds import bound_margins

    m, x, y = _rows(70)
    clf = estimator(build(m, max_batch=32))  # 70 rows: three chunks
    eps = np.resize(np.array([0.0, 0.01, 0.05], np.float32), 70)
    both, det = bound_margins(clf, x, eps, y=y, details=True)
    one = device_call(model_of("nonneg"), x, eps, y, INF, clip=(-INF, INF))
    assert np.array_equal(det["margin_ibp"].cpu().numpy(), one["margin_ibp"]) and np.array_equal(det["margin_crown"].cpu().numpy(), one["margin_crown"])
    assert np.array_equal(both.cpu().numpy(), np.maximum(one["margin_ibp"], one["margin_crown"]))
    assert np.array_equal(bound_margins(clf, x, eps, method="ibp", y=y).cpu().numpy(), one["margin_ibp"])
    assert np.array_equal(bound_margins(clf, torch.as_tensor(x).cuda(), 0.01, y=np.eye(5)[y]).cpu().numpy()[1::3], both.cpu().numpy()[1::3])
    with pytest.raises(ValueError):
        bound_margins(clf, x, -0.1)
    with pytest.raises(ValueError):
        bound_margins(clf, x, 0.1, norm=1)
    with pytest.raises(ValueError):
        bound_margins(clf, x, 0.1, method="alpha-crown")


@pytest.mark.parametrize("norm", NORMS)
def test_certified_radius_against_the_float64_driver(norm):
    from lipasr.bounds import bound_margins, certified_radius

    m, x, y = _rows()
    clf = estimator(model_of("nonneg"))
    eps_max, steps = 0.2 if norm == INF else 1.0, 10
    got = certified_radius(clf, x, norm=norm, eps_max=eps_max, steps=steps).cpu().numpy().astype(np.float64)
    want, _ = R.certified_radius(m, x, norm, (-INF, INF), y, eps_max, steps)
    step = eps_max * 2.0 ** -(steps - 1)
    print(f"norm {norm}: radii {np.sort(got)}; largest |device - float64| {np.abs(got - want).max():.3e}, one step {step:.3e}")
    assert (np.abs(got - want) <= step * (1 + 1e-6)).all()
    assert (got > 0).mean() >= 0.5
    # monotone: certified at eps, certified at eps / 2
    rows = got > 0
    for f in (1.0, 0.5):
        mm = bound_margins(clf, x[rows], (got[rows] * f).astype(np.float32), norm=norm).amin(dim=1).cpu().numpy()
        assert (mm > 0).all()
    # a wrong label gives 0
    wrong = (y + 1) % 5
    assert (certified_radius(clf, x, norm=norm, y=wrong, eps_max=eps_max, steps=3).cpu().numpy() == 0).all()


SANDWICH_GRID = (0.02, 0.06, 0.15, 0.4)


def test_every_pgd_flip_lies_beyond_the_certified_radius():
    from lipasr.attacks import ProjectedGradientDescent
    from lipasr.bounds import certified_radius

    m, x, y = _rows()
    # not vacuous: the float64 reference alone certifies at least half the rows at the smallest eps of the grid
    ref = R.bound_margins(m, x, np.full(len(x), SANDWICH_GRID[0]), INF, (-INF, INF), y).min(-1)
    assert (ref > 0).mean() >= 0.5
    clf = estimator(model_of("nonneg"))
    radius = certified_radius(clf, x, norm=INF, eps_max=SANDWICH_GRID[-1], steps=12).cpu().numpy()
    assert (radius >= SANDWICH_GRID[0]).mean() >= 0.5
    flips = 0
    for e in SANDWICH_GRID:
        adv = ProjectedGradientDescent(estimator=clf, eps=e, eps_step=e / 4, max_iter=20, norm=np.inf).generate(x)
        assert np.abs(adv - x).max() <= e + 2 * K.spacing32(np.abs(x).max() + e)  # x + delta is rounded to fp32 once
        flipped = clf.predict(adv).argmax(-1) != y
        flips += int(flipped.sum())
        print(f"eps {e}: PGD flipped {int(flipped.sum())} of {len(x)}, certified {(radius >= e).sum()}")
        assert (radius[flipped] < e).all()
    assert flips > 0


def test_get_robustness_radius_adds_only_bound_radius():
    from lipasr.extract_features_construct_dataset import get_robustness_radius

    m, x, y = _rows(8)
    clf = estimator(model_of("nonneg"))
    for norm in (2, np.inf):
        plain = get_robustness_radius(clf, x, norm=norm, max_iter=10)
        assert set(plain) == {"margin", "certified", "linear", "found", "flipped"} and (plain["certified"] is None) == (norm == np.inf)
        more = get_robustness_radius(clf, x, norm=norm, max_iter=10, bounds=dict(eps_max=0.5, steps=8, method="crown-ibp"))
        assert set(more) == set(plain) | {"bound_radius"}
        r = more["bound_radius"]
        assert r.dtype == np.float64 and r.shape == (8,) and (r >= 0).all() and (r > 0).any()
        assert (r[more["flipped"]] <= more["found"][more["flipped"]]).all()
        for k in plain:
            assert plain[k] is None and more[k] is None or np.array_equal(plain[k], more[k])


def test_attack_eval_certify_report(capsys):
    import lipasr.attack_eval as V
    from lipasr.attacks import ProjectedGradientDescent

    m, x, y = _rows(48)
    model = model_of("nonneg")
    models = {"constrained": model, "unconstrained": model}
    train, val, test = x[:16], x[16:32], x[32:]
    labels = np.eye(5)[y[32:]]
    grid = [0.02, 0.1, 0.4]
    capsys.readouterr()
    rep = V.certify_report(models, train, val, test, labels, norm=np.inf, standardize="after", grid=grid, steps=6)
    out = capsys.readouterr().out
    assert sum(line.startswith("Certified accuracy (crown-ibp, norm inf) over 16 test rows") for line in out.splitlines()) == 2 * len(grid)
    assert out.count("Median radius certified by bound propagation over 16 test rows") == 2 and "Lipschitz" not in out
    clf = estimator(model)
    for e, a in zip(grid, rep["constrained"]["certified_accuracy"]):
        adv = ProjectedGradientDescent(estimator=clf, eps=e, eps_step=e / 4, max_iter=20, norm=np.inf).generate(test)
        assert a <= float((clf.predict(adv).argmax(-1) == y[32:]).mean())
    assert rep["constrained"]["certified_accuracy"][0] > 0 and (np.diff(rep["constrained"]["certified_accuracy"]) <= 0).all()
    rep2 = V.certify_report(models, train, val, test, labels, norm=2, method="ibp", standardize="after", grid=grid, points=2, steps=4)
    out = capsys.readouterr().out
    assert len(rep2["constrained"]["certified_accuracy"]) == 2 and out.count("Median radius the Lipschitz bound certifies") == 2
    ibp = rep2["constrained"]["certified_accuracy"]
    assert (ibp <= V.certify_report(models, train, val, test, labels, norm=2, standardize="after", grid=grid, points=2, steps=4)["constrained"]["certified_accuracy"]).all()
    # radius_report prints bound_radius only when asked
    capsys.readouterr()
    V.radius_report(models, train, val, test, over="mfcc", standardize="after", norm=np.inf, max_iter=4)
    assert "bound propagation" not in capsys.readouterr().out
    r = V.radius_report(models, train, val, test, over="mfcc", standardize="after", norm=np.inf, max_iter=4, bounds=dict(eps_max=0.4, steps=6))
    assert "Radius certified by bound propagation over 16 test rows" in capsys.readouterr().out and r["constrained"]["bound_radius"].shape == (16,)
