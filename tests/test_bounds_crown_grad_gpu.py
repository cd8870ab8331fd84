"""CROWN-IBP certified training on the device: lipasr_mlp_bounds_crown_grad against the autograd oracle of
tests/bounds_crown_grad_ref.py at the tolerance of tests/test_bounds_crown_grad_cpu.py, against the host twin for equal values,
twice and at a shifted workspace for the same bits, launch counts on the reference shape; then the training step: beta_t = 0 is
the IBPCrossentropy step bit for bit, three certified steps track the composed float64 oracle, and CROWN-IBP training certifies on
the harder recipe what IBP training does not."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bounds_crown_grad_ref as CR
import bounds_ref as R
from helpers import build_model, dev, load_params, read_params, rel_err
from test_bounds_crown_grad_cpu import BETAS, CASES, check_against_oracle, inputs_of, layout_of
from test_bounds_gpu import REF_WIDTHS, build, device_call, estimator

import lipasr._native as N
import lipasr.keras as KS
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu

INF = float("inf")


@functools.lru_cache(maxsize=None)
def model_of(case):
    return build(CASES[case][0])


@functools.lru_cache(maxsize=None)
def device_forward(case):
    x, eps, y = inputs_of(case)
    return device_call(model_of(case), x, eps, y, INF, crown=True), y


def grad_call(model, fwd, y, beta, ws_offset=0, scale_old=0.0, scale_new=1.0, grads=None):
    """One lipasr_mlp_bounds_crown_grad on what a forward call wrote, the workspace ``ws_offset`` floats into its allocation."""
    b = len(y)
    need = C.c_size_t()
    N.check(N.lib.lipasr_mlp_bounds_crown_grad_workspace(model._plan, b, C.byref(need)))
    ws = torch.zeros(need.value + ws_offset, device="cuda")[ws_offset:]
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dt).contiguous()
    g = torch.zeros_like(model._params) if grads is None else t(grads)
    rows = torch.full((b,), 7.0, device="cuda")
    mi, mc, lo, hi, yt = t(fwd["margin_ibp"]), t(fwd["margin_crown"]), t(fwd["lo"]), t(fwd["hi"]), t(y, torch.int32)
    N.check(N.lib.lipasr_mlp_bounds_crown_grad(model._plan, N.ptr(model._params), N.ptr(model._bnstate), N.ptr(mi), N.ptr(mc), N.ptr(lo),
                                               N.ptr(hi), N.ptr(yt), b, beta, N.ptr(ws), need.value, scale_old, scale_new, N.ptr(g),
                                               N.ptr(rows), N.stream_ptr()))
    torch.cuda.synchronize()
    return {"grads": g.cpu().numpy(), "loss_rows": rows.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def device_grad(case, beta, ws_offset=0):
    fwd, y = device_forward(case)
    return grad_call(model_of(case), fwd, y, beta, ws_offset=ws_offset)


def host_grad_of(case, fwd, y, beta, **kw):
    m = CASES[case][0]
    params, state = R.pack(m, layout_of(m))
    return N.mlp_bounds_crown_grad_host(m["widths"], R.bn_flags(m), params, state, fwd["margin_ibp"], fwd["margin_crown"], fwd["lo"],
                                        fwd["hi"], y, beta, **kw)


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("case", list(CASES))
def test_device_against_autograd(case, beta):
    check_against_oracle(case, beta, device_grad(case, beta), "device")


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_host_twin(case, beta):
    fwd, y = device_forward(case)
    dev_out, twin = device_grad(case, beta), host_grad_of(case, fwd, y, beta)
    for k in dev_out:
        print(f"{case} beta {beta} {k}: max |device - host| {np.abs(dev_out[k].astype(np.float64) - twin[k]).max():.3e}")
    for k in dev_out:
        assert np.array_equal(dev_out[k], twin[k]), k


# M = batch x classes past one span of 1024 rows: (widths, BatchNorm layers, batch)
SPAN_CASES = {"second_span_26_rows": ([37, 33, 18, 5], (0, 1), 210), "second_span_1_row": ([37, 33, 18, 5], (0, 1), 205),
              "second_span_one_chunk": ([19, 40, 32], (0,), 33)}


@pytest.mark.parametrize("name", list(SPAN_CASES))
def test_device_equals_host_twin_across_spans(name):
    """Two spans of rows: cg_wgrad_kernel's second span starts at row 1024 and ends mid-chunk (26 rows, 1 row) or after exactly one
    chunk, and cg_wreduce_kernel and cg_finish_kernel add two partials each."""
    widths, bn, B = SPAN_CASES[name]
    m = R.make_model(widths, 2, bn=bn)
    assert 1024 < B * widths[-1] <= 2048
    x, eps, y = R.case_inputs(m, B, 8)
    model = build(m, max_batch=256)
    fwd = device_call(model, x, eps, y, INF, crown=True)
    got = grad_call(model, fwd, y, 1.0)
    params, state = R.pack(m, layout_of(m))
    twin = N.mlp_bounds_crown_grad_host(m["widths"], R.bn_flags(m), params, state, fwd["margin_ibp"], fwd["margin_crown"], fwd["lo"],
                                        fwd["hi"], y, 1.0)
    assert np.isfinite(twin["grads"]).all() and np.abs(twin["grads"]).max() > 0
    for k in got:
        assert np.array_equal(got[k], twin[k]), k


@pytest.mark.parametrize("case", ["signed70", "wide"])
def test_same_bits_twice_and_at_a_shifted_workspace(case):
    fwd, y = device_forward(case)
    a = device_grad(case, 0.5)
    assert same_bits(a, grad_call(model_of(case), fwd, y, 0.5)) and same_bits(a, device_grad(case, 0.5, 1))


def test_scale_old_and_beta_zero_on_the_device():
    from test_bounds_grad_gpu import grad_call as ibp_grad_call

    fwd, y = device_forward("signed70")
    m = CASES["signed70"][0]
    pre = np.random.default_rng(3).standard_normal(layout_of(m)[1]).astype(np.float32)
    got = grad_call(model_of("signed70"), fwd, y, 0.5, scale_old=0.75, scale_new=0.5 / 70, grads=pre)
    twin = host_grad_of("signed70", fwd, y, 0.5, scale_old=0.75, scale_new=0.5 / 70, grads=pre)
    assert np.array_equal(got["grads"], twin["grads"]) and not np.array_equal(got["grads"], device_grad("signed70", 0.5)["grads"])
    zero = grad_call(model_of("signed70"), fwd, y, 0.0, scale_old=0.75, scale_new=0.5 / 70, grads=pre)
    ibp = ibp_grad_call(model_of("signed70"), fwd, y, scale_old=0.75, scale_new=0.5 / 70, grads=pre)
    assert same_bits(zero, ibp)


def test_launch_counts_on_the_reference_shape():
    m = R.make_model(REF_WIDTHS, 9, bn=(0, 1, 2, 3, 4), signed=False, scale=0.5)
    model = build(m, max_batch=8)
    x = np.random.default_rng(5).standard_normal((2, 880)).astype(np.float32)
    y = R.forward(m, x).argmax(-1).astype(np.int32)
    fwd = device_call(model, x, np.full(2, 0.01, np.float32), y, INF, clip=(-INF, INF), crown=True)
    count = lambda: ([N.lib.lipasr_debug_bounds_crown_grad_launches(i) for i in range(len(N.BOUNDS_CROWN_GRAD_KERNELS))],
                     [N.lib.lipasr_debug_bounds_grad_launches(i) for i in range(len(N.BOUNDS_GRAD_KERNELS))])
    diff = lambda a, b: ([q - p for p, q in zip(a[0], b[0])], [q - p for p, q in zip(a[1], b[1])])
    L = len(REF_WIDTHS) - 1
    c0 = count()
    out = grad_call(model, fwd, y, 1.0)
    own, ibp = diff(c0, count())
    want = N.bounds_crown_grad_launches(L)
    assert own == [want[k] for k in N.BOUNDS_CROWN_GRAD_KERNELS] == [1, L - 1, L - 1, L - 1, L - 1, L - 1, L - 1, L - 1, 1]
    assert ibp == [N.bounds_grad_launches(L)[k] for k in N.BOUNDS_GRAD_KERNELS] and sum(own) + sum(ibp) == 10 * (L - 1) + 3
    assert np.isfinite(out["grads"]).all() and np.abs(out["grads"]).max() > 0
    c0 = count()
    grad_call(model, fwd, y, 0.0)
    own, ibp = diff(c0, count())
    assert sum(own) == 0 and sum(ibp) == 3 * (L - 1) + 1
    c0 = count()
    device_grad.__wrapped__("linear", 1.0)
    own, ibp = diff(c0, count())
    assert own == [1, 1, 0, 0, 0, 0, 0, 0, 1] and ibp == [2, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------- the training step
def _state(model):
    return [t.clone() for t in (model._params, model._adam_m, model._adam_v, model._bnstate, model._step)]


def test_beta_zero_is_the_ibp_step_bit_for_bit(cuda):
    from lipasr.bounds import CrownIBPCrossentropy, IBPCrossentropy

    spec = [P.LayerSpec(37, 33, True, 0.1, False), P.LayerSpec(33, 18, True, 0.1, True), P.LayerSpec(18, 5, False, 0.0, False)]
    p = P.init_params(spec, seed=4, dtype=np.float32)
    rng = np.random.default_rng(21)
    xs = rng.standard_normal((5, 70, 37)).astype(np.float32)
    ys = [P.to_categorical(rng.integers(0, 5, 70), 5) for _ in range(5)]
    states = []
    for loss in (IBPCrossentropy(0.1, kappa=0.5, warmup_steps=1, ramp_steps=2),
                 CrownIBPCrossentropy(0.1, kappa=0.5, warmup_steps=1, ramp_steps=2, beta_start=0.0, beta_end=0.0)):
        model = build_model(spec, max_batch=128, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        load_params(model, p)
        for x, y in zip(xs, ys):
            model.train_on_batch(dev(x), dev(y))
        torch.cuda.synchronize()
        states.append(_state(model))
        assert loss.step == 5 and "ws_crown" not in model._ibp_buffers
    assert all(torch.equal(a, b) for a, b in zip(*states))


def test_three_certified_steps_track_the_oracle(cuda):
    """tests/test_bounds_grad_gpu.py::test_three_certified_steps_track_the_oracle with the CROWN-IBP loss at beta 0.5: signed70's
    shape at batch 70, exact fp32, injected dropout masks, kappa 0.5 and eps 0.1 from the first step, the same bounds.  The robust
    gradient of the composed oracle is bounds_crown_grad_ref's (without the slack, 1e-5-sized, which these bounds absorb)."""
    from lipasr.bounds import CrownIBPCrossentropy

    spec = [P.LayerSpec(37, 33, True, 0.1, False), P.LayerSpec(33, 18, True, 0.1, False), P.LayerSpec(18, 5, False, 0.0, False)]
    p = P.init_params(spec, seed=6, dtype=np.float32)
    rng = np.random.default_rng(31)
    for l in (0, 1):
        p.gamma[l] = (1 + 0.2 * rng.standard_normal(spec[l].n_out)).astype(np.float32)
        p.beta[l] = (0.1 * rng.standard_normal(spec[l].n_out)).astype(np.float32)
        p.mov_mean[l] = (0.3 + 0.1 * rng.standard_normal(spec[l].n_out)).astype(np.float32)
        p.mov_var[l] = rng.uniform(0.5, 1.5, spec[l].n_out).astype(np.float32)
    loss = CrownIBPCrossentropy(0.1, kappa=0.5, beta_start=0.5, beta_end=0.5)
    loss.step = 1  # past the one-step ramp: every step below is a certified one
    model = build_model(spec, max_batch=128, compute_dtype="float32")
    model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
    load_params(model, p)
    p64, st, B = p.astype(np.float64), P.AdamState(), 70
    for step in range(3):
        eps_t, kappa_t = loss.schedule(loss.step)
        assert (eps_t, kappa_t, loss.beta_schedule(loss.step)) == (0.1, 0.5, 0.5)
        x = rng.standard_normal((B, 37)).astype(np.float32)
        labels = rng.integers(0, 5, B)
        y = P.to_categorical(labels, 5)
        masks = [((rng.uniform(size=(B, s.n_out)) > s.dropout) / (1 - s.dropout)).astype(np.float32) if s.dropout > 0 else None for s in spec]
        out = P.forward_backward(spec, p64, x.astype(np.float64), y.astype(np.float64), masks=masks, training=True)
        bn = [None if not s.bn else (p64.gamma[l], p64.beta[l], p64.mov_mean[l] * P.BN_MOMENTUM + out["stats"][l][0] * (1 - P.BN_MOMENTUM),
                                     p64.mov_var[l] * P.BN_MOMENTUM + out["stats"][l][1] * (1 - P.BN_MOMENTUM)) for l, s in enumerate(spec)]
        ref = {"widths": [37, 33, 18, 5], "W": p64.W, "b": p64.b, "bn": bn}
        rows, rob = CR.loss_and_grads(ref, x, np.full(B, eps_t), labels, 0.5, clip=(-INF, INF))
        mixed = {k: [None if a is None else (1 - kappa_t) * a + kappa_t / B * r for a, r in zip(out[k], rob[k])]
                 for k in ("dW", "db", "dgamma", "dbeta")}
        P.train_step(spec, p64, st, x.astype(np.float64), y.astype(np.float64), masks=masks, grads_override=mixed)
        model.train_on_batch(dev(x), dev(y), masks=[dev(k) if k is not None else None for k in masks])
        logged = float(model._loss_rows[:B].mean())
        want = (1 - kappa_t) * out["loss"] + kappa_t * rows.mean()
        print(f"step {step}: mixed loss {logged:.6f}, oracle {want:.6f}")
        assert abs(logged - want) < 1e-4 * max(1.0, abs(want))
    after = read_params(model, spec)
    for l in range(3):
        d = np.abs(after.W[l] - p64.W[l])
        print(f"layer {l}: |W - oracle| 0.9999 quantile {np.quantile(d, 0.9999):.3e}, max {d.max():.3e}")
        assert np.quantile(d, 0.9999) < 2e-4 and d.max() < 3e-3, (l, np.quantile(d, 0.9999), d.max())
        if spec[l].bn:
            assert rel_err(after.mov_mean[l], p64.mov_mean[l]) < 1e-4
            assert rel_err(after.mov_var[l], p64.mov_var[l]) < 1e-4
            assert np.abs(after.gamma[l] - p64.gamma[l]).max() < 2e-4
    assert int(model._step.item()) == 3 and loss.step == 4 and "ws_crown" in model._ibp_buffers


def test_crown_ibp_training_certifies_what_ibp_training_does_not(cuda):
    """The recipe of DESIGN.md, "CROWN-IBP certified training", seed 0: 10 blobs in 20 dimensions at noise 0.5, 20 -> 64 -> 32 -> 10
    with BatchNorm, Adam 1e-3, batch 64, 400 steps (50 warm-up, 200 ramp), kappa 1, eps 0.4, clip +-2.5; 512 fresh rows certified by
    method "crown-ibp" at eps 0.4.  The float64 trainer of bounds_crown_grad_ref gives clean 1.000 and certified 0.830 for CROWN-IBP
    at beta 1 throughout against 0.623 and 0.346 for IBP; the thresholds leave room for fp32 and for the widening."""
    from lipasr.bounds import CrownIBPCrossentropy, IBPCrossentropy, certified_accuracy

    spec = [P.LayerSpec(20, 64, True, 0.0, False), P.LayerSpec(64, 32, True, 0.0, False), P.LayerSpec(32, 10, False, 0.0, False)]
    xt, yt = CR.blobs(512, 999)
    batches = [CR.blobs(64, 10_000 + step) for step in range(400)]
    kw = dict(kappa=1.0, warmup_steps=50, ramp_steps=200, clip_values=(-2.5, 2.5))
    got = {}
    for name, loss in (("ibp", IBPCrossentropy(0.4, **kw)), ("crown-ibp", CrownIBPCrossentropy(0.4, beta_start=1.0, beta_end=1.0, **kw))):
        model = build_model(spec, max_batch=512, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        for x, y in batches:
            model.train_on_batch(dev(x), dev(P.to_categorical(y, 10)))
        clf = estimator(model)
        clean = float((clf.predict(xt).argmax(-1) == yt).mean())
        cert = float(certified_accuracy(clf, xt, yt, [0.4], method="crown-ibp", clip_values=(-2.5, 2.5))[0])
        got[name] = (clean, cert)
        print(f"{name}: clean accuracy {clean:.3f}, certified accuracy (crown-ibp) at eps 0.4 {cert:.3f}")
    assert got["crown-ibp"][0] >= 0.95 and got["crown-ibp"][1] >= 0.70 and got["crown-ibp"][1] >= got["ibp"][1] + 0.30
