"""The psychoacoustic kernels (csrc/psycho.hip) against the NumPy float64 restatement of tests/psycho_ref.py.

Every parity bound is 8 x the error of the SAME restatement evaluated in float32 on the CPU (the yardstick rule of
tests/test_wave_attacks_gpu.py): three bits for the packed pair transform, the tabulated twiddles and the device log10f / exp10f
against pocketfft and NumPy.  Each test prints the worst device error next to its bound; DESIGN.md records the lines."""
import numpy as np
import pytest
import torch

import psycho_ref as R

pytestmark = pytest.mark.gpu

CASES = [(sr, n, b) for sr in R.RATES for n in R.SIZES for b in (1, 3)]


def _dev(a, cuda):
    return torch.as_tensor(np.ascontiguousarray(a)).to(cuda)


@pytest.fixture(scope="module")
def maskers(cuda):
    from lipasr.psychoacoustic import PsychoacousticMasker

    ms = {(sr, by): PsychoacousticMasker(sample_rate=sr, bark_by=by) for sr in R.RATES for by in ("bin", "position")}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def clean(cuda, maskers):
    """Per case: the clips, the device PSD of them and the float64 / float32 restatement's."""
    out = {}
    for sr, n, b in CASES:
        x = R.clips(n, sr, b)
        psd, mx = maskers[(sr, "bin")].psd_device(_dev(x, cuda))
        out[(sr, n, b)] = dict(x=x, psd=psd.cpu().numpy(), mx=mx.cpu().numpy(), ref64=[R.psd(c.astype(np.float64)) for c in x],
                               ref32=[R.psd(c, np.float32) for c in x])
    return out


def _power(p):
    return 10.0 ** (np.asarray(p, dtype=np.float64) / 10.0)


def test_psd_matches_the_restatement(clean):
    rows = []
    for (sr, n, b), c in clean.items():
        assert c["psd"].shape == (b, R.n_frames(n), R.K) and np.isfinite(c["psd"]).all() and np.isfinite(c["mx"]).all()
        for u in range(b):
            p64, m64 = c["ref64"][u]
            p32, m32 = c["ref32"][u]
            if not c["x"][u].any():  # the silent clip
                assert np.all(c["psd"][u] == 96.0) and c["mx"][u] == -200.0
                continue
            ref = _power(p64)
            top = ref.max(axis=1)
            e = (np.abs(_power(c["psd"][u]) - ref).max(axis=1) / top).max()
            y = (np.abs(_power(p32) - ref).max(axis=1) / top).max()
            em = abs(_power(c["mx"][u]) - _power(m64)) / _power(m64)
            ym = abs(_power(m32) - _power(m64)) / _power(m64)
            rows.append(((sr, n, b, u), e, y, em, ym))
    yard, yard_m = max(r[2] for r in rows), max(r[4] for r in rows)
    print(f"psd: linear power per frame, worst device {max(r[1] for r in rows):.3e}, float32 restatement {yard:.3e}, bound {8 * yard:.3e}")
    print(f"psd_max: linear, worst device {max(r[3] for r in rows):.3e}, float32 restatement {yard_m:.3e}, bound {8 * yard_m:.3e}")
    for key, e, _, em, _ in rows:
        assert e <= 8 * yard, (key, e)
        assert em <= 8 * yard_m, (key, em)


def _theta_errors(theta_dev, t64, t32):
    """Worst relative error per bin of the device and of the float32 restatement; bins where theta is 0 must be 0."""
    zero = t64 == 0
    assert np.all(theta_dev[zero] == 0)
    rel = lambda a: (np.abs(a.astype(np.float64)[~zero] - t64[~zero]) / t64[~zero]).max()
    return rel(theta_dev), rel(t32)


@pytest.mark.parametrize("by", ("bin", "position"))
def test_threshold_on_the_devices_own_psd(clean, maskers, by, cuda):
    rows, total, left_out, zeros = [], 0, 0, 0
    for (sr, n, b), c in clean.items():
        theta, cnt = maskers[(sr, by)].threshold_device(_dev(c["psd"], cuda), return_counts=True)
        theta, cnt = theta.cpu().numpy(), cnt.cpu().numpy()
        assert np.isfinite(theta).all() and (theta >= 0).all()
        for u in range(b):
            t64, n64, margin = R.threshold(c["psd"][u].astype(np.float64), sr, by)
            t32, n32, _ = R.threshold(c["psd"][u], sr, by, np.float32)
            keep = margin >= R.MARGIN_DB
            total += len(keep)
            left_out += int((~keep).sum())
            zeros += int(((t64 == 0) & keep[:, None]).sum())
            assert np.array_equal(cnt[u][keep], n64[keep]), (sr, n, b, u, cnt[u], n64)
            same = keep & (n32 == n64)
            e, _ = _theta_errors(theta[u][keep], t64[keep], t32[keep])
            _, y = _theta_errors(theta[u][same], t64[same], t32[same])
            rows.append(((sr, n, b, u), e, y))
    yard = max(r[2] for r in rows)
    print(f"threshold {by}: {left_out} of {total} frames left out (margin < {R.MARGIN_DB} dB); theta relative per bin, worst device "
          f"{max(r[1] for r in rows):.3e}, float32 restatement {yard:.3e}, bound {8 * yard:.3e}; {zeros} bins with theta == 0 checked")
    assert left_out <= R.MAX_LEFT_OUT * total
    assert zeros > 0  # (the silent clip below 20 Hz: no ATH and no masker)
    for key, e, _ in rows:
        assert e <= 8 * yard, (key, e)


@pytest.mark.parametrize("by", ("bin", "position"))
def test_threshold_on_synthetic_psds(maskers, by, cuda):
    for sr in R.RATES:
        m = maskers[(sr, by)]
        ath = R.tables(sr)[2]
        saw = R.sawtooth(R.SAW_SEED[by])
        p = np.stack([saw, np.full(R.K, 30.0, dtype=np.float32), saw[::-1].copy()])[None]  # one clip of three frames
        theta, cnt = m.threshold_device(_dev(p, cuda), return_counts=True)
        theta, cnt = theta.cpu().numpy()[0], cnt.cpu().numpy()[0]
        t64, n64, margin = R.threshold(p[0].astype(np.float64), sr, by)
        t32, n32, _ = R.threshold(p[0], sr, by, np.float32)
        assert margin[0] >= 1e-3 and margin[1] == np.inf
        ok = margin >= R.MARGIN_DB
        assert ok[0] and ok[1]
        assert np.array_equal(cnt[ok], n64[ok]) and np.array_equal(n32[ok], n64[ok])
        e, y = _theta_errors(theta[ok], t64[ok], t32[ok])
        print(f"sawtooth {by} sr {sr}: maskers {cnt.tolist()} (511 candidates in frames 0 and 2), theta worst device {e:.3e}, float32 "
              f"restatement {y:.3e}, bound {8 * y:.3e}")
        assert e <= 8 * y
        # the flat frame: no masker, theta = 10^(ATH/10), 0 where the ATH is -inf
        fin = np.isfinite(ath)
        assert cnt[1] == 0 and np.all(theta[1][~fin] == 0)
        np.testing.assert_allclose(theta[1][fin], 10.0 ** (ath[fin] / 10.0), rtol=2.0 ** -23)


@pytest.fixture(scope="module")
def thresholds(clean):
    """Per case and clip: the restatement's float64 threshold and psd_max of the clean clip, rounded to what the device is given."""
    out = {}
    for (sr, n, b), c in clean.items():
        th = np.stack([R.threshold(c["ref64"][u][0], sr)[0] for u in range(b)]).astype(np.float32)
        out[(sr, n, b)] = (th, np.array([c["ref64"][u][1] for u in range(b)], dtype=np.float32))
    return out


def test_loss_and_gradient_match_the_restatement(clean, thresholds, maskers, cuda):
    rows, shares, exact = [], {}, 0
    for (sr, n, b), (th, mx) in thresholds.items():
        m = maskers[(sr, "bin")]
        th_t, mx_t = _dev(th, cuda), _dev(mx, cuda)
        last = R.HOP * (R.n_frames(n) - 1) + R.N
        for amp in R.AMPLITUDES:
            d = (np.float32(amp) * R.noise(n, b)).astype(np.float32)
            d_t = _dev(d, cuda)
            loss, g = m.loss_gradient_device(d_t, th_t, mx_t)
            loss2, g2 = m.loss_gradient_device(d_t, th_t, mx_t)
            loss3, none = m.loss_gradient_device(d_t, th_t, mx_t, need_grad=False)
            assert torch.equal(loss, loss2) and torch.equal(g, g2) and torch.equal(loss, loss3) and none is None
            loss, g = loss.double().cpu().numpy(), g.double().cpu().numpy()
            assert np.isfinite(loss).all() and np.isfinite(g).all()
            assert np.all(g[:, last:] == 0)
            for u in range(b):
                l64, g64, p64 = R.loss_grad(d[u].astype(np.float64), th[u].astype(np.float64), float(mx[u]), detail=True)
                l32, g32 = R.loss_grad(d[u], th[u], float(mx[u]), np.float32)
                if clean[(sr, n, b)]["x"][u].any():
                    shares.setdefault(amp, []).append((p64 > th[u]).mean())
                if l64 == 0:  # nothing over theta: the relative errors have no denominator; the result is exact instead
                    assert loss[u] == 0 and l32 == 0 and not g[u].any() and not g64.any()
                    exact += 1
                    continue
                errs = lambda l, gg: (abs(float(l) - l64) / l64, np.abs(gg - g64).max() / np.abs(g64).max(),
                                      np.linalg.norm(gg - g64) / np.linalg.norm(g64))
                rows.append(((sr, n, b, u, amp), errs(loss[u], g[u]), errs(l32, g32.astype(np.float64))))
    yard = [max(r[2][i] for r in rows) for i in range(3)]
    worst = [max(r[1][i] for r in rows) for i in range(3)]
    for amp, s in shares.items():
        print(f"share of bins over theta at amplitude {amp}: mean {100 * np.mean(s):.2f}%")
    print(f"loss_grad: {len(rows)} rows compared, {exact} rows with nothing over theta (loss and gradient exactly 0 on both sides)")
    for i, name in enumerate(("loss relative", "gradient inf-norm / max|g|", "gradient 2-norm")):
        print(f"loss_grad {name}: worst device {worst[i]:.3e}, float32 restatement {yard[i]:.3e}, bound {8 * yard[i]:.3e} "
              f"(device / yardstick {worst[i] / yard[i]:.2f})")
    for key, e, _ in rows:
        for i in range(3):
            assert e[i] <= 8 * yard[i], (key, i, e[i])


def test_nothing_over_the_threshold_gives_exact_zeros(clean, thresholds, maskers, cuda):
    for (sr, n, b), (th, mx) in thresholds.items():
        m = maskers[(sr, "bin")]
        live = [u for u in range(b) if clean[(sr, n, b)]["x"][u].any()]
        d = (np.float32(1e-15) * R.noise(n, b)).astype(np.float32)
        for u in live:  # the restatement agrees that nothing exceeds theta
            assert R.loss_grad(d[u].astype(np.float64), th[u].astype(np.float64), float(mx[u]))[0] == 0
        for dd, rows in ((d, live), (np.zeros_like(d), list(range(b)))):
            loss, g = m.loss_gradient_device(_dev(dd, cuda), _dev(th, cuda), _dev(mx, cuda))
            assert np.all(loss.cpu().numpy()[rows] == 0)
            assert np.all(g.cpu().numpy().view(np.uint32)[rows] == 0)  # +0.0, bit for bit


def test_step_kernel_against_its_restatement(maskers, cuda):
    m = maskers[(16000, "bin")]
    rng = np.random.default_rng(5)
    b, n = 3, 2600
    f = lambda s: (s * rng.standard_normal((b, n))).astype(np.float32)
    x0, delta, g_net, g_theta = np.clip(f(0.5), -1, 1), f(0.01), f(1.0), f(3.0)
    alpha = np.array([0.05, 0.5, 2.0], dtype=np.float32)
    eps = np.array([0.02, 0.005, 0.03], dtype=np.float32)
    for use_sign, gt, lr, clip in ((True, None, 0.004, (-1.0, 1.0)), (False, g_theta, 0.002, (-1.0, 1.0)), (False, g_theta, 0.002, (-0.3, 0.4))):
        d_t, xa_t = _dev(delta, cuda), torch.empty(b, n, device=cuda)
        m.step_device(d_t, xa_t, _dev(x0, cuda), _dev(g_net, cuda), None if gt is None else _dev(gt, cuda),
                      None if gt is None else _dev(alpha, cuda), _dev(eps, cuda), lr, use_sign, clip)
        d_ref, xa_ref = R.step(delta, x0, g_net, gt, alpha, eps, lr, use_sign, *clip)
        d_dev, xa_dev = d_t.cpu().numpy(), xa_t.cpu().numpy()
        t = g_net if gt is None else g_net + alpha[:, None] * gt
        big = np.maximum.reduce([np.abs(delta), np.abs(np.float32(lr) * t), np.abs(x0), np.abs(xa_ref)])
        tol = 2 * np.spacing(big.astype(np.float32))
        print(f"step sign={use_sign} clip={clip}: worst |delta - restatement| / tolerance {np.max(np.abs(d_dev - d_ref) / tol):.3f}, "
              f"x_adv {np.max(np.abs(xa_dev - xa_ref) / tol):.3f}")
        assert np.all(np.abs(d_dev - d_ref) <= tol) and np.all(np.abs(xa_dev - xa_ref) <= tol)
        assert xa_dev.min() >= clip[0] and xa_dev.max() <= clip[1]
        inner = (xa_dev > clip[0]) & (xa_dev < clip[1])
        assert np.all(np.abs(d_dev[inner]) <= eps[:, None].repeat(n, 1)[inner] + np.spacing(np.float32(1.0)))
        # each row's own eps binds somewhere, and the rows differ
        assert all(np.isclose(np.abs(d_dev[u][inner[u]]).max(), eps[u], rtol=0, atol=2e-7) for u in range(b))


# ---------------------------------------------------------------------------------------------- the attack
L = 44


@pytest.fixture(scope="module")
def attack_setup(cuda):
    """Four clips, a signed-glorot unconstrained classifier and a scaler fitted on the clips' features, as in
    tests/test_wave_attacks_gpu.py; per clip a target different from the prediction."""
    import mfcc_grad_ref as G
    from helpers import build_model, load_params
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from oracle import mlp_ref as P

    spec = P.vd_unconstrained_spec()
    p = P.init_params(spec, seed=3, nonneg_init=False)
    m = build_model(spec, max_batch=32)
    load_params(m, p)
    ex = MfccExtractor(16000, 16000, batch_max=8)
    x = torch.as_tensor(G.parity_clips(16000)).to(cuda).contiguous()
    feats = ex(x, L).double().cpu().numpy()
    mean, scale = feats.mean(axis=0), feats.std(axis=0)
    scale[scale == 0.0] = 1.0
    pred = m.predict_device(ex(x, L, torch.as_tensor(mean).to(cuda), torch.as_tensor(scale).to(cuda))).argmax(dim=1).cpu().numpy()
    y = G.onehot((pred + 1 + np.arange(4)) % 10, 10)
    yield dict(spec=spec, p64=p.astype(np.float64), model=m, ex=ex, x=x, y22=ex.resample(x), mean=mean, scale=scale, y=y)
    ex.close()


def _clf(s, domain):
    from lipasr import attacks as A

    return A.WaveformClassifier(s["model"], 10, extractor=s["ex"], utterance_length=L, mean=s["mean"], scale=s["scale"], domain=domain)


@pytest.mark.parametrize("domain", ("22k", "input"))
def test_attack_invariants(attack_setup, domain, cuda):
    from lipasr import attacks as A

    s = attack_setup
    clf = _clf(s, domain)
    x0 = s["y22"] if domain == "22k" else s["x"]
    keep = x0.clone()
    yt = torch.as_tensor(s["y"]).to(cuda)
    atk = A.ImperceptibleASR(clf, eps=0.05, learning_rate_1=0.005, learning_rate_2=2e-4, max_iter_1=20, max_iter_2=20,
                             num_iter_decrease_eps=5, num_iter_increase_alpha=5, num_iter_decrease_alpha=10)
    assert atk.masker.sample_rate == (22050 if domain == "22k" else 16000)  # masker=None: the domain's sample rate
    adv = atk.generate_device(x0, yt)
    assert torch.equal(x0, keep) and adv.data_ptr() != x0.data_ptr() and adv.shape == x0.shape
    assert torch.isfinite(adv).all() and float(adv.min()) >= -1.0 and float(adv.max()) <= 1.0
    d = (adv - x0).abs().amax(dim=1).cpu().numpy()
    print(f"imperceptible {domain}: success {atk.last_success.tolist()}, eps {atk.last_eps.tolist()}, max|delta| {d.tolist()}, "
          f"L_theta after stage 1 {atk.last_loss_theta_1.tolist()}, after stage 2 {atk.last_loss_theta.tolist()}")
    assert np.all(d <= atk.last_eps + np.spacing(np.float32(1.0))) and np.all(atk.last_eps <= np.float32(0.05))
    hit = (clf.predict_device(adv, logits=True).argmax(dim=1).cpu().numpy() == s["y"].argmax(axis=1))
    ok = atk.last_success
    assert ok.dtype == bool and ok.shape == (4,) and np.all(hit[ok])
    assert np.all(atk.last_loss_theta[ok] <= atk.last_loss_theta_1[ok])
    assert np.isfinite(atk.last_loss_theta).all() and np.isfinite(atk.last_loss_theta_1).all()
    # NumPy in, NumPy out; the input stays as it was
    xn = x0.cpu().numpy()
    xk = xn.copy()
    small = A.ImperceptibleASR(clf, eps=0.01, learning_rate_1=0.002, learning_rate_2=1e-4, max_iter_1=2, max_iter_2=1)
    an = small.generate(xn, s["y"])
    assert isinstance(an, np.ndarray) and an.shape == xn.shape and np.array_equal(xn, xk) and np.abs(an - xn).max() <= 0.01 + 1e-6


def test_attack_argument_errors(attack_setup, cuda):
    from lipasr import attacks as A
    from lipasr.psychoacoustic import PsychoacousticMasker

    s = attack_setup
    clf = _clf(s, "input")
    kw = dict(eps=0.01, learning_rate_1=0.002, learning_rate_2=1e-4)
    for drop in kw:  # no defaults for eps and the learning rates
        with pytest.raises(TypeError):
            A.ImperceptibleASR(clf, **{k: v for k, v in kw.items() if k != drop})
    atk = A.ImperceptibleASR(clf, masker=PsychoacousticMasker(sample_rate=16000, bark_by="position"), max_iter_1=1, max_iter_2=1, **kw)
    assert atk.masker.bark_by == "position"
    yt = torch.as_tensor(s["y"]).to(cuda)
    with pytest.raises(ValueError):
        atk.generate_device(s["x"], None)
    with pytest.raises(ValueError):
        atk.generate(s["x"].cpu().numpy(), None)
    with pytest.raises(ValueError):
        atk.generate_device(s["x"], yt, lengths=[16000] * 4)
    with pytest.raises(ValueError):
        atk.generate(s["x"].cpu().numpy(), s["y"], lengths=[16000] * 4)
    with pytest.raises(TypeError):
        A.ImperceptibleASR(A.TensorFlowV2Classifier(model=s["model"], nb_classes=10, input_shape=(880,)), **kw)
    with pytest.raises(ValueError):
        A.ImperceptibleASR(clf, eps=0.0, learning_rate_1=0.002, learning_rate_2=1e-4)


@pytest.mark.parametrize("domain", ("22k", "input"))
def test_one_stage2_iteration_equals_the_composed_step(attack_setup, domain, cuda):
    """x0 + delta after ONE stage-2 iteration from the stage-1 result, against the step composed on the CPU from the restatement's
    g_theta (on the device's own theta, so that both sides see the same hinge) and the float64 g_net of tests/mfcc_grad_ref.py.
    Bound: lr2 x (8 x the float32 oracle's error of each gradient, in the inf-norm), plus what float32 itself takes from the step:
    the device rounds delta - lr t (half an ulp of at most eps) and x0 + delta (half an ulp of at most 1) and the composed step
    rounds neither, which no gradient bound covers -- together under one ulp of 1."""
    import mfcc_grad_ref as G
    from lipasr import attacks as A
    from oracle import mlp_ref as P

    s = attack_setup
    clf = _clf(s, domain)
    x0 = s["y22"] if domain == "22k" else s["x"]
    sr = 22050 if domain == "22k" else 16000
    yt = torch.as_tensor(s["y"]).to(cuda)
    lr2, alpha = 5e-6, 0.05  # (a theta step of 1e-4 .. 1e-2: inside the ball for most samples, so the clamp does not hide it)
    atk = A.ImperceptibleASR(clf, eps=0.02, learning_rate_1=0.004, learning_rate_2=lr2, alpha=alpha, max_iter_1=10, max_iter_2=1,
                             num_iter_decrease_eps=5)
    atk.generate_device(x0, yt)
    theta, mx = atk.masker.prepare_device(x0.contiguous())
    theta, mx = theta.cpu().numpy(), mx.cpu().numpy()
    x0n, x1, got = x0.cpu().numpy(), atk.last_stage1.cpu().numpy(), atk.last_iterate.cpu().numpy()
    rows = []
    for i in range(4):
        d1 = x1[i] - x0n[i]
        _, gth = R.loss_grad(d1.astype(np.float64), theta[i].astype(np.float64), float(mx[i]))
        _, gth32 = R.loss_grad(d1, theta[i], float(mx[i]), np.float32)
        s64 = x1[i].astype(np.float64)
        kw = dict(scale=s["scale"], domain=domain)
        grads = []
        for dt in (torch.float64, torch.float32):
            f = G.features(torch.as_tensor(s64), mean=s["mean"], dtype=dt, **kw).double().numpy()
            gfeat = P.input_gradient_infer(s["spec"], s["p64"], f[None, :], s["y"][i:i + 1].astype(np.float64))[0]
            grads.append(np.asarray(G.vjp(s64, gfeat, dtype=dt, **kw), dtype=np.float64))
        gnet, gnet32 = grads
        dn = np.clip(d1.astype(np.float64) - lr2 * (gnet + alpha * gth), -atk.last_eps[i], atk.last_eps[i])
        want = np.clip(x0n[i] + dn, -1.0, 1.0)
        y_net, y_th = np.abs(gnet32 - gnet).max(), np.abs(gth32.astype(np.float64) - gth).max()
        bound = lr2 * 8 * (y_net + alpha * y_th) + np.spacing(np.float32(1.0))
        err = np.abs(got[i] - want).max()
        rows.append((i, err, bound, np.abs(lr2 * gnet).max(), np.abs(lr2 * alpha * gth).max()))
        print(f"stage-2 step {domain} clip {i}: |x_adv - composed| {err:.3e}, bound {bound:.3e}; step sizes: net {rows[-1][3]:.3e}, "
              f"theta {rows[-1][4]:.3e}")
    for i, err, bound, _, _ in rows:
        assert err <= bound, (i, err, bound)


def test_imperceptible_report_over_wav_files(attack_setup, tmp_path, capsys):
    """The evaluation entry behind ``python -m lipasr.attack_eval --attack white --kind imperceptible --over audio``."""
    import wave

    from lipasr import attack_eval as V

    s = attack_setup
    files = []
    for i in range(4):
        path = tmp_path / f"clip_{i}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(s["x"][i].cpu().numpy(), -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats = s["ex"](s["x"], L).double().cpu().numpy()
    models = {"constrained": s["model"], "unconstrained": s["model"]}
    labels = s["y"].astype(np.float32)
    out = V.imperceptible_report(models, feats, feats, feats, labels, files, eps=0.02, learning_rate_1=0.004, learning_rate_2=5e-6,
                                 max_iter_1=10, max_iter_2=10, num_iter_decrease_eps=5, num_iter_increase_alpha=5, num_iter_decrease_alpha=10)
    text = capsys.readouterr().out
    for name in models:
        r = out[name]
        assert 0.0 <= r["success"] <= 1.0 and np.isfinite(r["loss_theta_1"]) and np.isfinite(r["loss_theta_2"]) and r["snr_db"] > 0
        assert r["rows"]["success"].shape == (4,)
    assert out["constrained"]["success"] == out["unconstrained"]["success"]  # the same model twice, the same targets
    assert "Targeted success rate of the imperceptible attack" in text and "Mean masking loss L_theta" in text and "SNR" in text
    with pytest.raises(ValueError):
        V.imperceptible_report(models, feats, feats, feats, labels, None, eps=0.02, learning_rate_1=0.004, learning_rate_2=5e-6)
    with pytest.raises(ValueError):
        V.imperceptible_report(models, feats, feats, feats, labels, files, eps=0.02, learning_rate_1=0.004, learning_rate_2=5e-6, domain="mel")
