"""IBP certified training on the device: lipasr_mlp_bounds_grad against the autograd oracle of tests/bounds_grad_ref.py at the
tolerance of tests/test_bounds_grad_cpu.py, against the host twin for equal values, twice and at a shifted workspace for the same
bits, launch counts on the reference shape; then the training step: kappa_t = 0 is the plain step bit for bit, three certified
steps track the composed float64 oracle, and IBP training certifies what plain training does not."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bounds_grad_ref as G
import bounds_ref as R
from helpers import build_model, dev, load_params, read_params, rel_err
from test_bounds_gpu import REF_WIDTHS, build, device_call, estimator
from test_bounds_grad_cpu import CASES, check_against_oracle, layout_of

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
    m, B = CASES[case]
    x, eps, y = R.case_inputs(m, B, len(case))
    return device_call(model_of(case), x, eps, y, INF, crown=False), y


def grad_call(model, fwd, y, ws_offset=0, scale_old=0.0, scale_new=1.0, grads=None):
    """One lipasr_mlp_bounds_grad on what a forward call wrote, the workspace ``ws_offset`` floats into its allocation."""
    b = len(y)
    need = C.c_size_t()
    N.check(N.lib.lipasr_mlp_bounds_grad_workspace(model._plan, b, C.byref(need)))
    ws = torch.zeros(need.value + ws_offset, device="cuda")[ws_offset:]
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dt).contiguous()
    g = torch.zeros_like(model._params) if grads is None else t(grads)
    rows = torch.full((b,), 7.0, device="cuda")
    mt, lo, hi, yt = t(fwd["margin_ibp"]), t(fwd["lo"]), t(fwd["hi"]), t(y, torch.int32)
    N.check(N.lib.lipasr_mlp_bounds_grad(model._plan, N.ptr(model._params), N.ptr(model._bnstate), N.ptr(mt), N.ptr(lo), N.ptr(hi), N.ptr(yt), b,
                                         N.ptr(ws), need.value, scale_old, scale_new, N.ptr(g), N.ptr(rows), N.stream_ptr()))
    torch.cuda.synchronize()
    return {"grads": g.cpu().numpy(), "loss_rows": rows.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def device_grad(case, ws_offset=0):
    fwd, y = device_forward(case)
    return grad_call(model_of(case), fwd, y, ws_offset=ws_offset)


def host_grad_of(case, fwd, y, **kw):
    m = CASES[case][0]
    params, state = R.pack(m, layout_of(m))
    return N.mlp_bounds_grad_host(m["widths"], R.bn_flags(m), params, state, fwd["margin_ibp"], fwd["lo"], fwd["hi"], y, **kw)


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize("case", list(CASES))
def test_device_against_autograd(case):
    check_against_oracle(case, device_grad(case), "device")


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_host_twin(case):
    fwd, y = device_forward(case)
    dev_out, twin = device_grad(case), host_grad_of(case, fwd, y)
    for k in dev_out:
        print(f"{case} {k}: max |device - host| {np.abs(dev_out[k].astype(np.float64) - twin[k]).max():.3e}")
    for k in dev_out:
        assert np.array_equal(dev_out[k], twin[k]), k


@pytest.mark.parametrize("case", ["signed70", "wide"])
def test_same_bits_twice_and_at_a_shifted_workspace(case):
    fwd, y = device_forward(case)
    a = device_grad(case)
    assert same_bits(a, grad_call(model_of(case), fwd, y)) and same_bits(a, device_grad(case, 1))


def test_scale_old_on_the_device_equals_the_host_twin():
    fwd, y = device_forward("signed70")
    m = CASES["signed70"][0]
    lay = layout_of(m)
    pre = np.zeros(lay[1], np.float32)
    rng = np.random.default_rng(3)
    for _, o, n in G.segments(m, lay):
        pre[o:o + n] = rng.standard_normal(n)
    got = grad_call(model_of("signed70"), fwd, y, scale_old=0.75, scale_new=0.5 / 70, grads=pre)
    twin = host_grad_of("signed70", fwd, y, scale_old=0.75, scale_new=0.5 / 70, grads=pre)
    assert np.array_equal(got["grads"], twin["grads"]) and not np.array_equal(got["grads"], device_grad("signed70")["grads"])


def test_launch_counts_on_the_reference_shape():
    m = R.make_model(REF_WIDTHS, 9, bn=(0, 1, 2, 3, 4), signed=False, scale=0.5)
    model = build(m, max_batch=8)
    x = np.random.default_rng(5).standard_normal((2, 880)).astype(np.float32)
    y = R.forward(m, x).argmax(-1).astype(np.int32)
    fwd = device_call(model, x, np.full(2, 0.01, np.float32), y, INF, clip=(-INF, INF), crown=False)
    count = lambda: [N.lib.lipasr_debug_bounds_grad_launches(i) for i in range(len(N.BOUNDS_GRAD_KERNELS))]
    c0 = count()
    out = grad_call(model, fwd, y)
    c1 = count()
    L = len(REF_WIDTHS) - 1
    want = N.bounds_grad_launches(L)
    assert [b - a for a, b in zip(c0, c1)] == [want[k] for k in N.BOUNDS_GRAD_KERNELS] == [2, L - 1, L - 2, L - 1]
    assert sum(want.values()) == 3 * (L - 1) + 1 <= 3 * (L - 1) + 2
    assert np.isfinite(out["grads"]).all() and np.abs(out["grads"]).max() > 0
    one = model_of("linear")
    c0 = count()
    device_grad.__wrapped__("linear")
    assert [b - a for a, b in zip(c0, count())] == [2, 0, 0, 0] and one._widths == [7, 3]


# ------------------------------------------------------------------------------------------------------- the training step
def _state(model):
    return [t.clone() for t in (model._params, model._adam_m, model._adam_v, model._bnstate, model._step)]


def test_kappa_zero_is_the_plain_step_bit_for_bit(cuda):
    from lipasr.bounds import IBPCrossentropy

    spec = [P.LayerSpec(37, 33, True, 0.1, False), P.LayerSpec(33, 18, True, 0.1, True), P.LayerSpec(18, 5, False, 0.0, False)]
    p = P.init_params(spec, seed=4, dtype=np.float32)
    rng = np.random.default_rng(21)
    xs = rng.standard_normal((5, 70, 37)).astype(np.float32)
    ys = [P.to_categorical(rng.integers(0, 5, 70), 5) for _ in range(5)]
    states = []
    for loss in (KS.CategoricalCrossentropy(), IBPCrossentropy(0.1, kappa=0.5, warmup_steps=10)):
        model = build_model(spec, max_batch=128, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        load_params(model, p)
        for x, y in zip(xs, ys):
            model.train_on_batch(dev(x), dev(y))  # dropout on: the Philox masks depend on the seed and the step alone
        torch.cuda.synchronize()
        states.append(_state(model))
        assert getattr(loss, "step", 5) == 5 and getattr(model, "_ibp_buffers", None) is None
    assert all(torch.equal(a, b) for a, b in zip(*states))


def test_refusals_of_the_training_step(cuda):
    from lipasr.bounds import IBPCrossentropy
    from lipasr.pipeline import TrainPipeline

    spec = [P.LayerSpec(37, 33, True, 0.0, False), P.LayerSpec(33, 5, False, 0.0, False)]
    model = build_model(spec, max_batch=16, compute_dtype="float32")
    model.compile(optimizer="adam", loss=IBPCrossentropy(0.1), metrics=["accuracy"])
    with pytest.raises(NotImplementedError, match="TrainPipeline"):
        TrainPipeline(model, batch=16)
    model._dp = object()
    try:
        with pytest.raises(NotImplementedError, match="DataParallel"):
            model.train_on_batch(dev(np.zeros((4, 37))), dev(np.eye(5)[:4]))
    finally:
        model._dp = None
    # a model compiled anew after its pipeline was built is refused where the step runs
    from lipasr.train_constraints import get_model

    ref = get_model(max_batch=16)
    ref.compile(optimizer="adam", loss=KS.CategoricalCrossentropy(), metrics=["accuracy"])
    pipe = TrainPipeline(ref, batch=16, use_graph=False)
    try:
        ref.compile(optimizer="adam", loss=IBPCrossentropy(0.1), metrics=["accuracy"])
        with pytest.raises(NotImplementedError, match="TrainPipeline"):
            pipe.step(None, dev(np.eye(10)[np.zeros(16, int)]), features=dev(np.zeros((16, 880))))
    finally:
        pipe.close()


def test_three_certified_steps_track_the_oracle(cuda):
    """signed70's shape at batch 70, exact fp32, injected dropout masks, kappa 0.5 and eps 0.1 from the first step: the bounds of
    tests/test_mlp_gpu.py::test_n_train_steps_track_the_oracle on the movement of the weights, the moving statistics and gamma.
    The oracle is composed: the plain gradient of oracle.mlp_ref, the robust one of bounds_grad_ref on the running statistics that
    the step's forward pass has just updated, Adam through mlp_ref.train_step."""
    from lipasr.bounds import IBPCrossentropy

    spec = [P.LayerSpec(37, 33, True, 0.1, False), P.LayerSpec(33, 18, True, 0.1, False), P.LayerSpec(18, 5, False, 0.0, False)]
    p = P.init_params(spec, seed=6, dtype=np.float32)
    rng = np.random.default_rng(31)
    for l in (0, 1):
        p.gamma[l] = (1 + 0.2 * rng.standard_normal(spec[l].n_out)).astype(np.float32)
        p.beta[l] = (0.1 * rng.standard_normal(spec[l].n_out)).astype(np.float32)
        p.mov_mean[l] = (0.3 + 0.1 * rng.standard_normal(spec[l].n_out)).astype(np.float32)
        p.mov_var[l] = rng.uniform(0.5, 1.5, spec[l].n_out).astype(np.float32)
    loss = IBPCrossentropy(0.1, kappa=0.5)
    loss.step = 1  # past the one-step ramp: every step below is a certified one
    model = build_model(spec, max_batch=128, compute_dtype="float32")
    model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
    load_params(model, p)
    p64, st, B = p.astype(np.float64), P.AdamState(), 70
    for step in range(3):
        eps_t, kappa_t = loss.schedule(loss.step)
        assert (eps_t, kappa_t) == (0.1, 0.5)
        x = rng.standard_normal((B, 37)).astype(np.float32)
        labels = rng.integers(0, 5, B)
        y = P.to_categorical(labels, 5)
        masks = [((rng.uniform(size=(B, s.n_out)) > s.dropout) / (1 - s.dropout)).astype(np.float32) if s.dropout > 0 else None for s in spec]
        out = P.forward_backward(spec, p64, x.astype(np.float64), y.astype(np.float64), masks=masks, training=True)
        bn = [None if not s.bn else (p64.gamma[l], p64.beta[l], p64.mov_mean[l] * P.BN_MOMENTUM + out["stats"][l][0] * (1 - P.BN_MOMENTUM),
                                     p64.mov_var[l] * P.BN_MOMENTUM + out["stats"][l][1] * (1 - P.BN_MOMENTUM)) for l, s in enumerate(spec)]
        ref = {"widths": [37, 33, 18, 5], "W": p64.W, "b": p64.b, "bn": bn}
        rows, rob = G.loss_and_grads(ref, x, np.full(B, eps_t), labels, clip=(-INF, INF))
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
    assert int(model._step.item()) == 3 and loss.step == 4


def test_ibp_training_certifies_what_plain_training_does_not(cuda):
    """The recipe of DESIGN.md, "Certified training", seed 0: 4 blobs in 20 dimensions, 20 -> 32 -> 16 -> 4 with BatchNorm, Adam
    1e-3, batch 64, 300 steps (50 warm-up, 150 ramp), kappa 0.5, eps 0.2; certified accuracy by IBP at eps 0.2 on 512 fresh rows.
    The float64 trainer of bounds_grad_ref gives 0.996 against 0.000 at clean accuracy 1.000; half of that gain is asked for."""
    from lipasr.bounds import IBPCrossentropy, certified_accuracy

    spec = [P.LayerSpec(20, 32, True, 0.0, False), P.LayerSpec(32, 16, True, 0.0, False), P.LayerSpec(16, 4, False, 0.0, False)]
    xt, yt = G.blobs(512, 77)
    batches = [G.blobs(64, 10_000 + step) for step in range(300)]
    got = {}
    for name, loss in (("ibp", IBPCrossentropy(0.2, kappa=0.5, warmup_steps=50, ramp_steps=150, clip_values=(-2.5, 2.5))),
                       ("plain", KS.CategoricalCrossentropy())):
        model = build_model(spec, max_batch=512, compute_dtype="float32")
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        for x, y in batches:
            model.train_on_batch(dev(x), dev(P.to_categorical(y, 4)))
        clf = estimator(model)
        clean = float((clf.predict(xt).argmax(-1) == yt).mean())
        cert = float(certified_accuracy(clf, xt, yt, [0.2], method="ibp", clip_values=(-2.5, 2.5))[0])
        got[name] = (clean, cert)
        print(f"{name}: clean accuracy {clean:.3f}, IBP-certified accuracy at eps 0.2 {cert:.3f}")
    assert got["ibp"][1] >= 0.5 and got["ibp"][1] >= got["plain"][1] + 0.5 and got["ibp"][0] >= 0.9
