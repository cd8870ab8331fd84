"""GPU suite of training for randomized smoothing: lipasr_smooth_loss against the float64 restatement and its host twin, the
training step's seam (lipasr_mlp_train_fwd / _bwd) against the plain step, the two losses of lipasr.smoothing against composed
calls and a float64 trainer, refusals, launch counts, the functional recipe of DESIGN.md and the step times."""
import ctypes as C

import numpy as np
import pytest
import torch

import smooth_loss_ref as SR
from helpers import build_model, dev, load_params, read_params, rel_err
from test_smooth_train_cpu import BETA, GAMMA, LAM, SIGMA, all_cases, case, check_against_ref

import lipasr._native as N
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu

SPEC = [P.LayerSpec(37, 33, True, 0.1, False), P.LayerSpec(33, 18, True, 0.1, False), P.LayerSpec(18, 5, False, 0.0, False)]


def device_loss(z, y, draws, sigma, lam, gamma, beta, scale):
    from lipasr.smoothing import smooth_loss

    zt, yt = dev(z), torch.as_tensor(y, dtype=torch.int32, device="cuda")
    out = {"dz": torch.full_like(zt, 7.0)}
    out.update({k: torch.full((len(y),), 7.0, device="cuda") for k in ("loss", "correct", "radius")})
    smooth_loss(zt, yt, draws, sigma, lam, gamma, beta, scale, out["dz"], out["loss"], out["correct"], out["radius"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_device_loss_against_restatement_and_host_twin(cuda):
    for shape, zs, seed in all_cases():
        z, y, sc = case(shape, zs, seed)
        ref = SR.smooth_loss_ref(z, y, shape[1], SIGMA, LAM, GAMMA, BETA, sc)
        got = device_loss(z, y, shape[1], SIGMA, LAM, GAMMA, BETA, sc)
        check_against_ref(got, ref, ("device", shape, zs))
        again = device_loss(z, y, shape[1], SIGMA, LAM, GAMMA, BETA, sc)
        assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got), (shape, zs, "two runs differ")
        host = N.smooth_loss_host(z, y, shape[1], SIGMA, LAM, GAMMA, BETA, sc)
        # the twin shares the arithmetic text: what separates the two is libm's last places, far inside the bound against float64
        twin = {k: host[k].astype(np.float64) for k in host}
        twin.update(dz_c=ref["dz_c"], dz_r=ref["dz_r"])
        check_against_ref(got, twin, ("device against host twin", shape, zs))
    # a poisoned clip on the device: NaN in its own rows only
    z, y, sc = case((4, 7, 3), 3.0, 11)
    clean = device_loss(z, y, 7, SIGMA, LAM, GAMMA, BETA, sc)
    z[1 * 7 + 3, 2] = np.nan
    y[3] = -1
    got = device_loss(z, y, 7, SIGMA, LAM, GAMMA, BETA, sc)
    ok = np.r_[0:7, 14:21]
    assert np.array_equal(got["dz"][ok], clean["dz"][ok]) and np.isnan(got["dz"][7:14]).all() and np.isnan(got["dz"][21:]).all()
    assert np.isnan(got["loss"][[1, 3]]).all() and np.array_equal(got["loss"][[0, 2]], clean["loss"][[0, 2]])
    assert not got["correct"][[1, 3]].any() and not got["radius"][[1, 3]].any()


def _state(model):
    return [t.clone() for t in (model._params, model._adam_m, model._adam_v, model._bnstate, model._step)]


def _seam_model(compute, fuse):
    model = build_model(SPEC, max_batch=128, compute_dtype=compute)
    load_params(model, P.init_params(SPEC, seed=4, dtype=np.float32))
    N.check(N.lib.lipasr_mlp_set_fuse_bn(model._plan, fuse))
    return model


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("compute", ["float32", "float16x2"])
def test_seam_reproduces_the_plain_step_bit_for_bit(cuda, compute, fuse):
    """lipasr_mlp_train_fwd, dz = (p - y) * (1 / B) with torch, lipasr_mlp_train_bwd(dz_bound = 1 / B) against
    lipasr_mlp_train_fwd_bwd: logits, bnstate and grads bit for bit, Philox dropout at the same seed and step.  The p are the
    probabilities the forward pass leaves in the plan (stage 6), which the test first shows to be the plain call's ``probs`` bit for
    bit; torch's own softmax may differ from the epilogue's in the last place, so it is not what feeds dz."""
    B = 70
    rng = np.random.default_rng(21)
    x, y = dev(rng.standard_normal((B, 37))), dev(P.to_categorical(rng.integers(0, 5, B), 5))
    plain = _seam_model(compute, fuse)
    probs = torch.zeros(B, 5, device="cuda")
    plain.train_fwd_bwd(x, y, probs=probs)
    logits_plain, dz_plain = torch.zeros(B, 5, device="cuda"), torch.zeros(B, 5, device="cuda")
    N.check(N.lib.lipasr_debug_mlp_stage(plain._plan, 2, 5, B, N.ptr(logits_plain), N.stream_ptr()))
    N.check(N.lib.lipasr_debug_mlp_stage(plain._plan, 2, 3, B, N.ptr(dz_plain), N.stream_ptr()))
    seam = _seam_model(compute, fuse)
    cfg = seam._dropout_cfg(None, True)
    logits, p_seam = torch.zeros(B, 5, device="cuda"), torch.zeros(B, 5, device="cuda")
    N.check(N.lib.lipasr_mlp_train_fwd(seam._plan, N.ptr(seam._params), N.ptr(seam._bnstate), N.ptr(x), B, C.byref(cfg), N.ptr(logits),
                                       N.stream_ptr()))
    N.check(N.lib.lipasr_debug_mlp_stage(seam._plan, 2, 6, B, N.ptr(p_seam), N.stream_ptr()))
    assert torch.equal(logits, logits_plain) and torch.equal(p_seam, probs) and torch.equal(seam._bnstate, plain._bnstate)
    for layer in (0, 1):  # what the backward pass will read: activations, BatchNorm outputs, saved statistics
        for which, n in ((0, B * SPEC[layer].n_out), (1, B * SPEC[layer].n_out), (2, 2 * SPEC[layer].n_out)):
            a, b = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
            N.check(N.lib.lipasr_debug_mlp_stage(plain._plan, layer, which, B, N.ptr(a), N.stream_ptr()))
            N.check(N.lib.lipasr_debug_mlp_stage(seam._plan, layer, which, B, N.ptr(b), N.stream_ptr()))
            assert torch.equal(a, b), (layer, which)
    inv = float(np.float32(1.0 / B))
    dz = ((p_seam - y) * inv).contiguous()
    assert torch.equal(dz, dz_plain)
    N.check(N.lib.lipasr_mlp_train_bwd(seam._plan, N.ptr(seam._params), N.ptr(x), N.ptr(dz), B, inv, C.byref(cfg), N.ptr(seam._grads),
                                       N.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(seam._grads, plain._grads)
    assert bool(seam._grads.abs().max() > 0)


def test_gaussian_at_sigma_zero_is_the_plain_step_bit_for_bit(cuda):
    from lipasr import keras as K
    from lipasr.smoothing import GaussianCrossentropy

    p = P.init_params(SPEC, seed=4, dtype=np.float32)
    rng = np.random.default_rng(21)
    xs = rng.standard_normal((5, 70, 37)).astype(np.float32)
    ys = [P.to_categorical(rng.integers(0, 5, 70), 5) for _ in range(5)]
    states = []
    for loss in (K.CategoricalCrossentropy(), GaussianCrossentropy(0.0, draws=1)):
        model = build_model(SPEC, max_batch=128, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        load_params(model, p)
        for x, y in zip(xs, ys):
            model.train_on_batch(dev(x), dev(y))
        torch.cuda.synchronize()
        states.append(_state(model))
    assert loss.step == 5 and not hasattr(model, "_smooth_buffers")
    assert all(torch.equal(a, b) for a, b in zip(*states))


@pytest.mark.parametrize("compute", ["float32", "float16x2"])
def test_gaussian_step_is_expand_then_the_plain_step(cuda, compute):
    """pins the counter layout: the copies of step t are lipasr_smooth_expand's at clip0 = 0, draw0 = t * draws"""
    from lipasr import keras as K
    from lipasr.smoothing import GaussianCrossentropy, smooth_expand

    p = P.init_params(SPEC, seed=4, dtype=np.float32)
    rng = np.random.default_rng(22)
    x, y = dev(rng.standard_normal((24, 37))), dev(P.to_categorical(rng.integers(0, 5, 24), 5))
    loss = GaussianCrossentropy(0.3, draws=4, seed=9)
    loss.step = 3
    a = build_model(SPEC, max_batch=128, compute_dtype=compute)
    a.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
    load_params(a, p)
    a.train_on_batch(x, y)
    b = build_model(SPEC, max_batch=128, compute_dtype=compute)
    load_params(b, p)
    noisy = smooth_expand(x, 4, 0.3, 9, clip0=0, draw0=12)
    b.train_fwd_bwd(noisy, y.repeat_interleave(4, dim=0))
    rows, right = b._loss_rows[:96].clone(), b._correct_rows[:96].clone()
    b.apply_adam()
    torch.cuda.synchronize()
    assert loss.step == 4 and all(torch.equal(s, t) for s, t in zip(_state(a), _state(b)))
    assert bool((noisy.view(24, 4, 37) - x[:, None, :]).abs().mean() > 0.1)  # the copies are noisy
    assert torch.allclose(a._loss_rows[:24], rows.view(24, 4).mean(dim=1)) and torch.allclose(a._correct_rows[:24], right.view(24, 4).mean(dim=1))


def _random_bn(p, rng):
    for l in (0, 1):
        p.gamma[l] = (1 + 0.2 * rng.standard_normal(SPEC[l].n_out)).astype(np.float32)
        p.beta[l] = (0.1 * rng.standard_normal(SPEC[l].n_out)).astype(np.float32)
        p.mov_mean[l] = (0.3 + 0.1 * rng.standard_normal(SPEC[l].n_out)).astype(np.float32)
        p.mov_var[l] = rng.uniform(0.5, 1.5, SPEC[l].n_out).astype(np.float32)


def _check_tracks(model, p64, steps):
    """the bounds of tests/test_mlp_gpu.py::test_n_train_steps_track_the_oracle"""
    after = read_params(model, SPEC)
    for l in range(3):
        d = np.abs(after.W[l] - p64.W[l])
        print(f"layer {l}: |W - oracle| 0.9999 quantile {np.quantile(d, 0.9999):.3e}, max {d.max():.3e}")
        assert np.quantile(d, 0.9999) < 2e-4 and d.max() < 3e-3, (l, np.quantile(d, 0.9999), d.max())
        if SPEC[l].bn:
            assert rel_err(after.mov_mean[l], p64.mov_mean[l]) < 1e-4
            assert rel_err(after.mov_var[l], p64.mov_var[l]) < 1e-4
            assert np.abs(after.gamma[l] - p64.gamma[l]).max() < 2e-4
    assert int(model._step.item()) == steps


def test_three_macer_steps_track_the_float64_trainer(cuda):
    """16 clips x 4 draws, injected dropout masks, lam 12 from the first step.  The noisy rows are read back from
    lipasr_smooth_expand and fed to the float64 autograd trainer (tests/smooth_loss_ref.py), Adam and the moving statistics through
    oracle.mlp_ref.train_step as the IBP test composes it; the loss bound is that of the certified-training tests (1e-4 relative)."""
    from lipasr.smoothing import MACERCrossentropy, smooth_expand

    rng = np.random.default_rng(31)
    p = P.init_params(SPEC, seed=6, dtype=np.float32)
    _random_bn(p, rng)
    loss = MACERCrossentropy(0.25, draws=4, lam=12.0, gamma=8.0, beta=16.0, warmup_steps=0, seed=5)
    model = build_model(SPEC, max_batch=128, compute_dtype="float32")
    model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
    load_params(model, p)
    p64, st, B, m = p.astype(np.float64), P.AdamState(), 16, 4
    active = 0
    for step in range(3):
        x = rng.standard_normal((B, 37)).astype(np.float32)
        labels = rng.integers(0, 5, B)
        masks = [((rng.uniform(size=(B * m, s.n_out)) > s.dropout) / (1 - s.dropout)).astype(np.float32) if s.dropout > 0 else None for s in SPEC]
        noisy = smooth_expand(dev(x), m, 0.25, 5, clip0=0, draw0=step * m).cpu().numpy().astype(np.float64)
        grads, rows = SR.torch_grads(SPEC, p64, noisy, labels, m, 0.25, 12.0, 8.0, 16.0, masks=masks)
        plain_rows = SR.torch_grads(SPEC, p64, noisy, labels, m, 0.25, 0.0, 8.0, 16.0, masks=masks)[1]
        active += int((rows > plain_rows + 1e-9).sum())
        P.train_step(SPEC, p64, st, noisy, P.to_categorical(np.repeat(labels, m), 5).astype(np.float64), masks=masks, grads_override=grads)
        model.train_on_batch(dev(x), dev(P.to_categorical(labels, 5)), masks=[dev(k) if k is not None else None for k in masks])
        logged, want = float(model._loss_rows[:B].mean()), float(rows.mean())
        print(f"step {step}: MACER loss {logged:.6f}, float64 trainer {want:.6f}")
        assert abs(logged - want) < 1e-4 * max(1.0, abs(want))
    assert active > 0  # the robust term took part
    _check_tracks(model, p64, 3)
    assert loss.step == 3


def test_macer_without_noise_and_lambda_tracks_the_plain_loss(cuda):
    """MACERCrossentropy(sigma 0, lam 0, draws 1) is plain cross-entropy through the seam and the fp64 loss kernel: three steps stay
    within the oracle-tracking bounds of the plain loss's own float64 oracle (not bit-equal: the loss gradient is rounded once from
    fp64 here, computed in fp32 there)."""
    from lipasr.smoothing import MACERCrossentropy

    rng = np.random.default_rng(33)
    p = P.init_params(SPEC, seed=6, dtype=np.float32)
    _random_bn(p, rng)
    model = build_model(SPEC, max_batch=128, compute_dtype="float32")
    model.compile(optimizer="adam", loss=MACERCrossentropy(0.0, draws=1, lam=0.0), metrics=["accuracy"])
    load_params(model, p)
    p64, st, B = p.astype(np.float64), P.AdamState(), 70
    for step in range(3):
        x = rng.standard_normal((B, 37)).astype(np.float32)
        y = P.to_categorical(rng.integers(0, 5, B), 5)
        masks = [((rng.uniform(size=(B, s.n_out)) > s.dropout) / (1 - s.dropout)).astype(np.float32) if s.dropout > 0 else None for s in SPEC]
        out = P.train_step(SPEC, p64, st, x.astype(np.float64), y.astype(np.float64), masks=masks)
        model.train_on_batch(dev(x), dev(y), masks=[dev(k) if k is not None else None for k in masks])
        logged = float(model._loss_rows[:B].mean())
        assert abs(logged - out["loss"]) < 1e-4 * max(1.0, abs(out["loss"]))
        assert float(model._correct_rows[:B].mean()) == pytest.approx(float((out["logits"].argmax(1) == y.argmax(1)).mean()))
    _check_tracks(model, p64, 3)


def test_refusals(cuda):
    from lipasr.pipeline import TrainPipeline
    from lipasr.smoothing import GaussianCrossentropy, MACERCrossentropy
    from lipasr.train_constraints import add_certified_arguments, add_smooth_arguments, smooth_loss
    import argparse

    for bad in (dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma=0.5, draws=0), dict(sigma=0.5, draws=65), dict(sigma=0.5, clip_values=(1, 0))):
        with pytest.raises(ValueError):
            GaussianCrossentropy(**bad)
    for bad in (dict(lam=-1.0), dict(gamma=0.0), dict(beta=0.0), dict(beta=float("nan")), dict(warmup_steps=-1)):
        with pytest.raises(ValueError):
            MACERCrossentropy(0.5, **bad)
    assert MACERCrossentropy(0.5, lam=3.0, warmup_steps=2).schedule(1) == 0.0 and MACERCrossentropy(0.5, lam=3.0, warmup_steps=2).schedule(2) == 3.0
    x, y = dev(np.zeros((40, 37))), dev(P.to_categorical(np.zeros(40, dtype=int), 5))
    for loss in (GaussianCrossentropy(0.5, draws=4), MACERCrossentropy(0.5, draws=4)):
        model = build_model(SPEC, max_batch=128, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        before = _state(model)
        with pytest.raises(ValueError, match=r"40 clips x 4 draws = 160 .* 128"):
            model.train_on_batch(x, y)
        assert all(torch.equal(a, b) for a, b in zip(before, _state(model)))
        model._dp = object()
        with pytest.raises(NotImplementedError, match="DataParallel"):
            model.train_on_batch(x[:8], y[:8])
        model._dp = None
        with pytest.raises(NotImplementedError, match="TrainPipeline"):
            TrainPipeline._refuse_certified(model)
    half = build_model(SPEC, max_batch=128, compute_dtype="float16x2")
    half.compile(optimizer="adam", loss=MACERCrossentropy(0.5, draws=4), metrics=["accuracy"])
    with pytest.raises(NotImplementedError, match="float32"):
        half.train_on_batch(x[:8], y[:8])
    ap = add_smooth_arguments(add_certified_arguments(argparse.ArgumentParser()))
    with pytest.raises(SystemExit):
        smooth_loss(ap.parse_args(["--smooth-sigma", "0.5", "--certified-eps", "0.1"]), ap)
    assert smooth_loss(ap.parse_args([]), ap) is None
    got = smooth_loss(ap.parse_args(["--smooth-sigma", "0.5", "--smooth-method", "macer", "--smooth-warmup", "7"]), ap)
    assert isinstance(got, MACERCrossentropy) and (got.sigma, got.draws, got.warmup_steps) == (0.5, 16, 7)


def _all_counters():
    lib = N.lib
    out = {("k2", k): lib.lipasr_debug_k2_launches(k) for k in range(9)}
    for key in np.ndindex(6, 2, 2, 2, 3, 12):
        v = lib.lipasr_debug_gemm_launches(*(int(i) for i in key))
        if v >= 0:
            out[("gemm",) + key] = v
    for fam in range(3):
        for arith in range(3):
            v = lib.lipasr_debug_group_launches(fam, arith, -1)
            if v >= 0:
                out[("group", fam, arith)] = v
    return out


def _moved(before):
    return {k: v - before[k] for k, v in _all_counters().items() if v != before[k]}


def test_a_macer_step_launches_the_plain_step_plus_expand_and_loss(cuda):
    from lipasr import keras as K
    from lipasr.smoothing import MACERCrossentropy

    rng = np.random.default_rng(3)
    x, y = dev(rng.standard_normal((16, 37))), dev(P.to_categorical(rng.integers(0, 5, 16), 5))
    big = dev(rng.standard_normal((64, 37)))
    plain = build_model(SPEC, max_batch=128, compute_dtype="float32")
    macer = build_model(SPEC, max_batch=128, compute_dtype="float32")
    macer.compile(optimizer="adam", loss=MACERCrossentropy(0.5, draws=4), metrics=["accuracy"])
    c0 = _all_counters()
    plain.train_on_batch(big, y.repeat_interleave(4, dim=0))
    want = _moved(c0)
    own = [N.lib.lipasr_debug_smooth_loss_launches(k) for k in range(2)]
    c1 = _all_counters()
    macer.train_on_batch(x, y)
    torch.cuda.synchronize()
    assert _moved(c1) == want and sum(want.values()) >= 6
    assert [N.lib.lipasr_debug_smooth_loss_launches(k) - own[k] for k in range(2)] == [1, 1]


# The float64 CPU trainer's average certified radii of the recipe (tests/smooth_loss_ref.py: train_cpu, acr_numpy; DESIGN.md,
# "Training for smoothing"), seeds 0, 1, 2 per method
CPU_ACR = {"plain": (0.6032, 0.6407, 0.6405), "gaussian": (0.6563, 0.6775, 0.6852), "macer": (0.6692, 0.6724, 0.6728)}


def test_training_for_smoothing_raises_the_certified_radius(cuda):
    """The recipe of DESIGN.md, seed 0, trained on the device; every score within its method's CPU seed range widened on each side by
    that range's own width.  Ordering: the CPU trainer's seed ranges are disjoint for plain < Gaussian and plain < MACER, and those
    two are asserted.  MACER's range lies INSIDE Gaussian's at this size (300 steps, 250 of them with the robust term; the blobs
    closer or sigma 1.0 did not separate them either, DESIGN.md has the numbers), so no order between the two is asserted."""
    from lipasr import keras as K
    from lipasr.attacks import TensorFlowV2Classifier
    from lipasr.smoothing import GaussianCrossentropy, MACERCrossentropy, Smooth

    cfg = SR.BLOB
    spec = SR.blob_spec()
    xt, yt = SR.blobs(cfg["rows"], 999)
    losses = {"plain": K.CategoricalCrossentropy(), "gaussian": GaussianCrossentropy(cfg["sigma"], draws=cfg["draws"]),
              "macer": MACERCrossentropy(cfg["sigma"], draws=cfg["draws"], lam=cfg["lam"], gamma=cfg["gamma"], beta=cfg["beta"],
                                         warmup_steps=cfg["warmup"])}
    got = {}
    for name, loss in losses.items():
        model = build_model(spec, max_batch=1024, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        load_params(model, P.init_params(spec, seed=0, dtype=np.float32))
        for step in range(cfg["steps"]):
            x, y = SR.blobs(cfg["batch"], 10_000 + step)
            model.train_on_batch(dev(x), dev(P.to_categorical(y, 4)))
        clf = TensorFlowV2Classifier(model=model, nb_classes=4, input_shape=(20,))
        res = Smooth(clf, cfg["sigma"], seed=1).certify(xt, n0=cfg["n0"], n=cfg["n"], alpha=cfg["alpha"])
        got[name] = float(np.where(res["class"] == yt, res["radius"], 0.0).mean())
        lo, hi = min(CPU_ACR[name]), max(CPU_ACR[name])
        print(f"{name}: average certified radius {got[name]:.4f}; CPU trainer, seeds 0-2: [{lo:.4f}, {hi:.4f}]")
    for name, acr in CPU_ACR.items():
        lo, hi = min(acr), max(acr)
        assert lo - (hi - lo) <= got[name] <= hi + (hi - lo), (name, got[name], lo, hi)
    assert got["plain"] < got["gaussian"] and got["plain"] < got["macer"], got


def test_step_times(cuda):
    """Printed with -s, no gate: the reference widths at 64 clips x 16 draws in exact fp32, lipasr_timer_*, 20 steps after 5."""
    from lipasr import keras as K
    from lipasr.smoothing import GaussianCrossentropy, MACERCrossentropy, smooth_loss

    spec = P.vd_constrained_spec()
    rng = np.random.default_rng(0)
    x64, y64 = dev(rng.standard_normal((64, 880))), dev(P.to_categorical(rng.integers(0, 10, 64), 10))
    x1k, y1k = dev(rng.standard_normal((1024, 880))), dev(P.to_categorical(rng.integers(0, 10, 1024), 10))
    h = N.get_handle(0)
    tid = C.c_int()
    N.check(N.lib.lipasr_timer_create(h.h, C.byref(tid)))

    def timed(fn):
        for _ in range(5):
            fn()
        N.check(N.lib.lipasr_timer_start(h.h, tid.value, N.stream_ptr()))
        for _ in range(20):
            fn()
        N.check(N.lib.lipasr_timer_stop(h.h, tid.value, N.stream_ptr()))
        torch.cuda.synchronize()
        ms = C.c_float()
        N.check(N.lib.lipasr_timer_elapsed_ms(h.h, tid.value, C.byref(ms)))
        return ms.value / 20 * 1e3

    out = {}
    for name, loss, (x, y) in (("plain step, 1024 rows", K.CategoricalCrossentropy(), (x1k, y1k)),
                               ("Gaussian step, 64 x 16", GaussianCrossentropy(0.5, draws=16), (x64, y64)),
                               ("MACER step, 64 x 16", MACERCrossentropy(0.5, draws=16), (x64, y64))):
        model = build_model(spec, max_batch=1024, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        out[name] = timed(lambda: model.train_on_batch(x, y))
    z = dev(rng.standard_normal((1024, 10)) * 3)
    lab = torch.as_tensor(rng.integers(0, 10, 64), dtype=torch.int32, device="cuda")
    dz, rows = torch.zeros_like(z), torch.zeros(64, device="cuda")
    out["lipasr_smooth_loss alone, 64 x 16 x 10"] = timed(lambda: smooth_loss(z, lab, 16, 0.5, 12.0, 8.0, 16.0, 1 / 64, dz, rows))
    for k, v in out.items():
        print(f"{k}: {v:.1f} us")
    assert all(v > 0 for v in out.values())
