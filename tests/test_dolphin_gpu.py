"""DolphinAttack on the device (lipasr.dolphin, csrc/dolphin.hip) against the SciPy restatement of tests/dolphin_ref.py.

Yardstick: every parity test evaluates the oracle chain in float64 (the truth) and in float32 (what plain fp32 arithmetic of the
same graph loses) on the CPU; a device figure may be at most 8 x the worst float32-oracle figure of the same batch and quantity
-- the factor tests/test_wave_attacks_gpu.py gives "same graph, different fp32 association".  Figures: |v - v64|inf / |v64|inf,
|s - s64|inf (the peak is 1), the relative error of the two peaks, |r - r64|inf / |r64|inf, each the worst over the clips with
at least 257 samples; a one-sample clip is checked for finiteness and exact zeros past its end only.

Shapes: rows of 4100 samples (no multiple of 64 or of 4: 64 whole chunks of the band-pass scan and a partial one, nine
workgroups of the decimator with a partial last one), five clips of 4100, 1000, 1, 257 and 4099 samples; one test at 16000 x 64.
"""
import wave

import numpy as np
import pytest
import torch

import dolphin_ref as D

pytestmark = pytest.mark.gpu

N_MAX, LENS, FACTOR = 4100, [4100, 1000, 1, 257, 4099], 8.0


def _signals(n_rows, n):
    # (in this order the one-sample clip of LENS is a chirp, and the quiet noise gets 1000 and 4099 samples)
    make = [lambda k: D.voiced(n, 140.0 + 7 * k, seed=2 + k), lambda k: D.quiet_noise(n, seed=3 + k), lambda k: D.chirp(n, seed=1 + k)]
    return np.stack([make[k % 3](k) for k in range(n_rows)]).astype(np.float32)


def _oracle(X, lens, **kw):
    """-> {dtype: [(v, s, peaks, r) per clip]} on each clip's valid part"""
    return {dt: [D.chain(X[u, :n].astype(np.float64), dt, **kw) for u, n in enumerate(lens)] for dt in (np.float64, np.float32)}


def _figures(got, ref64, lens):
    """got / ref64: per clip (v, s, peaks, r) with None for a quantity that was not computed -> worst figure per quantity"""
    fig = {}
    for u, n in enumerate(lens):
        if n < 257:
            continue
        v, s, pk, r = got[u]
        v64, s64, pk64, r64 = ref64[u]
        if v is not None:
            fig["v"] = max(fig.get("v", 0.0), np.abs(v[:n] - v64).max() / np.abs(v64).max())
        if s is not None:
            fig["s"] = max(fig.get("s", 0.0), np.abs(s[:12 * n] - s64).max())
        if pk is not None:
            fig["peaks"] = max(fig.get("peaks", 0.0), (np.abs(np.asarray(pk, dtype=np.float64) - pk64) / pk64).max())
        if r is not None:
            fig["r"] = max(fig.get("r", 0.0), np.abs(r[:n] - r64).max() / np.abs(r64).max())
    return fig


def _check(what, dev, ora):
    for k in dev:
        print(f"{what}: {k}: device {dev[k]:.3e}, float32 oracle {ora[k]:.3e}, ratio {dev[k] / ora[k]:.3f}")
    for k in dev:
        assert dev[k] <= FACTOR * ora[k], (what, k, dev[k], ora[k])


def _lens_t(lens, dev):
    return torch.as_tensor(np.asarray(lens, dtype=np.int32)).to(dev)


@pytest.fixture(scope="module")
def batch5(cuda):
    X = _signals(5, N_MAX)
    ora = _oracle(X, LENS)
    return X, ora


@pytest.fixture(scope="module")
def attack(cuda):
    from lipasr.dolphin import DolphinAttack

    da = DolphinAttack(16000, N_MAX, 5)
    yield da
    da.close()


def _np(t):
    return t.cpu().numpy()


def test_bandpass_parity(cuda, batch5, attack):
    X, ora = batch5
    v = _np(attack.bandpass(torch.as_tensor(X).to(cuda), _lens_t(LENS, cuda)))
    dev = _figures([(v[u], None, None, None) for u in range(5)], ora[np.float64], LENS)
    _check("band-pass", dev, _figures([(o[0], None, None, None) for o in ora[np.float32]], ora[np.float64], LENS))
    assert np.isfinite(v).all() and all(np.all(v[u, n:] == 0) for u, n in enumerate(LENS))


@pytest.mark.parametrize("carrier_hz", [30000, 25000])
def test_generate_parity(cuda, batch5, carrier_hz):
    from lipasr.dolphin import DolphinAttack

    X, ora = batch5
    if carrier_hz != 30000:
        ora = _oracle(X, LENS, carrier_hz=carrier_hz)
    da = DolphinAttack(16000, N_MAX, 5, carrier_hz=carrier_hz)
    s, pk = da.generate(torch.as_tensor(X).to(cuda), _lens_t(LENS, cuda), return_peaks=True)
    s, pk = _np(s), _np(pk)
    da.close()
    assert s.shape == (5, 12 * N_MAX) and pk.shape == (5, 2)
    dev = _figures([(None, s[u], pk[u], None) for u in range(5)], ora[np.float64], LENS)
    _check(f"generate at {carrier_hz} Hz", dev, _figures([(None, o[1], o[2], None) for o in ora[np.float32]], ora[np.float64], LENS))
    assert np.isfinite(s).all() and np.isfinite(pk).all()
    for u, n in enumerate(LENS):
        assert np.all(s[u, 12 * n:] == 0)
        assert np.abs(s[u, :12 * n]).max() == 1.0  # peak 2


def test_record_parity_on_foreign_buffer(cuda, attack):
    """record() on a 192 kHz buffer that generate() did not make: tones at 29 and 31 kHz (the microphone's square puts their
    difference at 2 kHz) plus noise."""
    k = np.arange(12 * N_MAX)
    rng = np.random.default_rng(11)
    buf = np.stack([0.4 * np.sin(2 * np.pi * 29000 * k / 192000 + u) + 0.4 * np.sin(2 * np.pi * 31000 * k / 192000) +
                    0.05 * rng.standard_normal(len(k)) for u in range(5)]).astype(np.float32)
    r = _np(attack.record(torch.as_tensor(buf).to(cuda), a1=1.0, a2=0.5, lengths=_lens_t(LENS, cuda)))
    ref = {dt: [(None, None, None, D.record(buf[u, :12 * n].astype(dt), 1.0, 0.5, dt)) for u, n in enumerate(LENS)] for dt in (np.float64, np.float32)}
    dev = _figures([(None, None, None, r[u]) for u in range(5)], ref[np.float64], LENS)
    _check("record", dev, _figures(ref[np.float32], ref[np.float64], LENS))
    assert np.isfinite(r).all() and all(np.all(r[u, n:] == 0) for u, n in enumerate(LENS))


def test_fused_parity(cuda, batch5, attack):
    """generate_recorded against the float64 oracle, and against generate followed by record, at the same bound."""
    X, ora = batch5
    xt, lt = torch.as_tensor(X).to(cuda), _lens_t(LENS, cuda)
    r = _np(attack.generate_recorded(xt, lt, a1=1.0, a2=0.5))
    two = _np(attack.record(attack.generate(xt, lt), 1.0, 0.5, lengths=lt))
    yard = _figures([(None, None, None, o[3]) for o in ora[np.float32]], ora[np.float64], LENS)
    _check("fused", _figures([(None, None, None, r[u]) for u in range(5)], ora[np.float64], LENS), yard)
    _check("fused against generate + record", _figures([(None, None, None, r[u]) for u in range(5)],
                                                       [(None, None, None, two[u, :n].astype(np.float64)) for u, n in enumerate(LENS)], LENS), yard)
    print("fused == generate + record bit for bit:", np.array_equal(r, two))
    assert np.isfinite(r).all() and all(np.all(r[u, n:] == 0) for u, n in enumerate(LENS))


def test_ragged_batch_equals_single_launches(cuda, batch5):
    """Every clip is bit-identical to a launch of that clip alone; what follows a clip in its row (NaN here) is never read and
    every output is finite, exactly 0 past the clip's end."""
    from lipasr.dolphin import DolphinAttack

    X, _ = batch5
    Xn = X.copy()
    for u, n in enumerate(LENS):
        Xn[u, n:] = np.nan
    da, one = DolphinAttack(16000, N_MAX, 5), DolphinAttack(16000, N_MAX, 1)
    xt, lt = torch.as_tensor(Xn).to(cuda), _lens_t(LENS, cuda)
    v, (s, pk), r = da.bandpass(xt, lt), da.generate(xt, lt, return_peaks=True), da.generate_recorded(xt, lt)
    buf = s.clone()  # the ultrasound itself, NaN-filled past each clip, for record()
    for u, n in enumerate(LENS):
        buf[u, 12 * n:] = float("nan")
    rr = da.record(buf, lengths=lt)
    for t in (v, s, pk, r, rr):
        assert torch.isfinite(t).all()
    for u, n in enumerate(LENS):
        assert torch.all(v[u, n:] == 0) and torch.all(s[u, 12 * n:] == 0) and torch.all(r[u, n:] == 0)
        x1, l1 = xt[u:u + 1].contiguous(), lt[u:u + 1].contiguous()
        s1, pk1 = one.generate(x1, l1, return_peaks=True)
        assert torch.equal(one.bandpass(x1, l1)[0], v[u]) and torch.equal(s1[0], s[u]) and torch.equal(pk1[0], pk[u])
        assert torch.equal(one.generate_recorded(x1, l1)[0], r[u])
        assert torch.equal(one.record(buf[u:u + 1].contiguous(), lengths=l1)[0], rr[u])
    da.close()
    one.close()


def test_two_calls_give_the_same_bits(cuda, batch5, attack):
    X, _ = batch5
    xt, lt = torch.as_tensor(X).to(cuda), _lens_t(LENS, cuda)
    a = (attack.bandpass(xt, lt), attack.generate(xt, lt), attack.generate_recorded(xt, lt))
    b = (attack.bandpass(xt, lt), attack.generate(xt, lt), attack.generate_recorded(xt, lt))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_silent_clip_gives_the_pure_carrier(cuda, attack):
    X = np.zeros((5, N_MAX), dtype=np.float32)
    X[1] = _signals(1, N_MAX)[0]
    xt = torch.as_tensor(X).to(cuda)
    s, pk = attack.generate(xt, return_peaks=True)
    r = attack.generate_recorded(xt)
    assert torch.isfinite(s).all() and torch.isfinite(r).all() and torch.isfinite(pk).all()
    cos = D.carrier(12 * N_MAX, 30000, np.float64)
    assert np.abs(_np(s[0]).astype(np.float64) - cos).max() <= 1e-6
    assert _np(pk)[0, 0] == 0 and abs(_np(pk)[0, 1] - 0.001) <= 1e-9


def test_full_size(cuda):
    """16000 x 64: parity of the recorded clips, the recorded clips through the MFCC extractor, and the demodulation property on
    the device: the recorded clip follows the voice at carrier level 1 and not at the reference's 0.001."""
    from lipasr.dolphin import DolphinAttack
    from lipasr.extract_features_construct_dataset import MfccExtractor

    n, b = 16000, 64
    X = _signals(b, n)
    lens = [n] * b
    ora = _oracle(X, lens)
    xt = torch.as_tensor(X).to(cuda)
    da = DolphinAttack(16000, n, b)
    r = da.generate_recorded(xt)
    v = _np(da.bandpass(xt))
    da.close()
    rn = _np(r)
    _check("full size", _figures([(None, None, None, rn[u]) for u in range(b)], ora[np.float64], lens),
           _figures([(None, None, None, o[3]) for o in ora[np.float32]], ora[np.float64], lens))
    ex = MfccExtractor(16000, n, b)
    assert torch.isfinite(ex(r, 44)).all()
    ex.close()
    da = DolphinAttack(16000, n, b, carrier_level=1.0)
    r1 = _np(da.generate_recorded(xt))
    da.close()
    # the property is one of signals whose square does not resemble them: the chirps of the batch (every third row), the signal it
    # is recorded for on the oracle in tests/test_dolphin_cpu.py -- the square of a harmonic stack holds the stack's own harmonics
    chirps = range(2, b, 3)
    hi = [D.demod_correlation(r1[u], v[u]) for u in chirps]
    lo = [D.demod_correlation(rn[u], v[u]) for u in chirps]
    print(f"correlation with the voice: >= {min(hi):.4f} at carrier level 1, <= {max(lo):.4f} at 0.001")
    assert min(hi) >= 0.9 and max(lo) <= 0.2


def test_error_codes(cuda):
    import lipasr._native as N
    from lipasr.dolphin import DolphinAttack

    with pytest.raises(N.LipasrError) as e:
        DolphinAttack(8000, N_MAX, 5)
    assert e.value.code == N.EUNSUPPORTED and "16000" in str(e.value)
    for hz in (7000, 89000, 30000.5):
        with pytest.raises(ValueError, match="carrier_hz"):
            DolphinAttack(16000, N_MAX, 5, carrier_hz=hz)
    with pytest.raises(ValueError, match="carrier_level"):
        DolphinAttack(16000, N_MAX, 5, carrier_level=-0.5)
    da = DolphinAttack(16000, N_MAX, 2)
    x = torch.zeros(3, N_MAX, device=cuda)
    for call in (lambda: da.bandpass(x), lambda: da.generate(x), lambda: da.generate_recorded(x),
                 lambda: da.record(torch.zeros(3, 12 * N_MAX, device=cuda))):
        with pytest.raises(ValueError, match="batch"):
            call()
    da.close()
    with pytest.raises(RuntimeError, match="after close"):
        da.bandpass(x[:2].contiguous())
    assert N.lib.lipasr_dolphin_bandpass(None, N.ptr(x), None, 1, N.ptr(x), None) == N.EINVAL  # lifetime: a plan that is gone


def _write_wav(path, x, sr):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((np.clip(x, -1, 1) * 32767.0).astype("<i2").tobytes())


def test_dolphin_sweep(cuda, tmp_path, capsys):
    """attack_eval.dolphin_sweep on 16 synthetic files and two small models: shapes, probabilities, and agreement with
    black_box_sweep(over="audio") at sigma 0 when the files themselves go through the sweep's extraction."""
    from lipasr import attack_eval as V
    from lipasr import extract_features_construct_dataset as E
    from lipasr import keras as K
    from lipasr import train_constraints as T
    from lipasr.synth import synth_clips

    waves, labels = synth_clips(64, seed=21)
    feats = E.mfcc(waves[:48]).cpu().numpy().astype(np.float64)
    train_data, val_data, test_data = feats[:36], feats[36:48], E.mfcc(waves[48:]).cpu().numpy().astype(np.float64)
    files = []
    for k in range(16):
        files.append(str(tmp_path / f"{k:02d}.wav"))
        _write_wav(files[-1], waves[48 + k], 16000)
    onehot = K.to_categorical(labels[48:], 10)
    tr = V.A.standardize_dataset(train_data, val_data, test_data)[0]
    models = {}
    for name, build in (("constrained", T.get_model), ("unconstrained", T.get_model_unconstrained)):
        K.reset_layer_names()
        m = build(max_batch=64)
        m.compile(optimizer="adam", loss=K.CategoricalCrossentropy(), metrics=["accuracy"])
        m.fit(K.Dataset.from_tensor_slices((tr, K.to_categorical(labels[:36], 10))).batch(36), epochs=4, verbose=0)
        models[name] = m
    grid, acc = V.dolphin_sweep(models, train_data, val_data, test_data, onehot, files, grid=[None, 0.001, 1.0])
    assert grid == [None, 0.001, 1.0] and set(acc) == {"constrained", "unconstrained"}
    for k in acc:
        assert acc[k].shape == (3,) and np.all(np.isfinite(acc[k])) and np.all((acc[k] >= 0) & (acc[k] <= 1))
    _, clean = V.black_box_sweep(models, train_data, val_data, test_data, onehot, kind="simple", over="audio", test_filenames=files, grid=[0])
    for k in acc:
        assert acc[k][0] == clean[k][0]
    grid, acc = V.dolphin_sweep(models, train_data, val_data, test_data, onehot, files, points=2, limit=8)
    assert grid == V.DOLPHIN_CARRIER_LEVELS[:2] and all(len(a) == 2 for a in acc.values())
    _write_wav(tmp_path / "8k.wav", waves[0][::2], 8000)
    with pytest.raises(ValueError, match="16 kHz"):
        V.dolphin_sweep(models, train_data, val_data, test_data, onehot, files + [str(tmp_path / "8k.wav")])
    assert "Accuracy on DolphinAttack recordings" in capsys.readouterr().out
