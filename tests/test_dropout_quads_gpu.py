"""The dropout masks do not depend on how the epilogues draw them, and the Adam kernel's "buffer free" signal.

Dropout keeps element e of a layer's [batch][width] activations when u01(o[e & 3]) > rate, o = Philox4x32-10 with key = the model's
seed and counter = (e >> 2, layer, step).  The epilogues walk a row in groups of four columns; a group whose first index is a
multiple of 4 shares its counter, and since this change it is drawn with ONE generator call (csrc/gemm.h: dropout_mult4) where it
took four before; whatever is not aligned (a width that is no multiple of 4, a ragged last group) keeps the call per element.

  * CPU: the NumPy restatement of the generator below reproduces the two known-answer vectors published with Random123
    (kat_vectors: counter and key all zero, counter and key all ones), and the restated mask rule has the structure the kernels rely on.
  * GPU: one training step with Philox dropout against the same step with `masks=` (mode 2: the kernels read the multipliers from
    memory) built by that restatement for the same (seed, layer, step): gradients, loss rows, correct rows and BatchNorm state
    bitwise equal, then Adam and a second step (step = 1 enters the counter), on every epilogue that applies dropout; each case
    asserts with the launch counters that the instance it is about really ran.
  * GPU: ten pipeline steps whose "buffer free" hand-off rides on the Adam kernel against the same steps on events.
"""
import numpy as np
import pytest
import torch

from helpers import build_model, dev, load_params
from oracle import mlp_ref as P
from philox_ref import philox_np

gpu = pytest.mark.gpu

FRAG4, FRAG16, LDS, RING, RING_X1, RING2 = range(6)
KINDS = ("FRAG4", "FRAG16", "LDS", "RING", "RING_X1", "RING2")
EPI_BIAS_RELU, EPI_BIAS_RELU_STATS, EPI_DH_STATS, EPI_DZ_NOBN, EPI_BIAS_RELU_BNX, EPI_DH_BNX = 2, 6, 7, 8, 10, 11
KNOB_NO_RING, KNOB_NO_X1 = 32, 512

# ---------------------------------------------------------------------------------------------
# the generator and the mask rule, restated
# ---------------------------------------------------------------------------------------------
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars) of one shape, key: (k0, k1) -> the four uint32 outputs."""
    seed = (int(key[0]) & 0xFFFFFFFF) | ((int(key[1]) & 0xFFFFFFFF) << 32)
    return [x.astype(np.uint32) for x in philox_np(seed, *ctr)]


def dropout_mask(seed, layer, step, rows, cols, rate):
    """The multipliers (0 or 1 / (1 - rate), float32) of a [rows][cols] activation: element e = row * cols + col."""
    e = np.arange(rows * cols, dtype=np.uint64)
    q = e >> np.uint64(2)
    o = philox4x32_10((q & MASK32, q >> np.uint64(32), np.uint64(layer), np.uint64(step)), (seed & 0xFFFFFFFF, seed >> 32))
    x = np.choose((e & np.uint64(3)).astype(np.int64), o)
    u = ((x >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(1.0 / 16777216.0)  # uniform in (0, 1], exact in float32
    rate = np.float32(rate)
    keep = np.float32(1.0) / (np.float32(1.0) - rate)
    return np.where(u > rate, keep, np.float32(0.0)).astype(np.float32).reshape(rows, cols)


def test_philox_restatement_against_known_answers():
    """(no GPU) The two Philox4x32-10 vectors of Random123's kat_vectors, and the mask rule's structure."""
    got = philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    got = philox4x32_10((f, f, f, f), (f, f))
    assert [int(v) for v in got] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # vectorised == one by one, counters above 2^32 included
    ctr = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7], dtype=np.uint64)
    many = philox4x32_10((ctr & MASK32, ctr >> np.uint64(32), 3, 9), (0x5EED0000, 0x12))
    for i, c in enumerate(ctr):
        one = philox4x32_10((int(c) & f, int(c) >> 32, 3, 9), (0x5EED0000, 0x12))
        assert [int(v[i]) for v in many] == [int(v) for v in one]
    # the mask rule: values 0 or 1 / (1 - rate); the share kept is 1 - rate; the four elements of an aligned group are the four
    # outputs of ONE counter, in order; layer and step enter the counter
    m = dropout_mask(0x5EED0000, 1, 0, 64, 96, 0.4)
    assert set(np.unique(m)) == {np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(0.4))}
    assert abs((m > 0).mean() - 0.6) < 4 * np.sqrt(0.24 / m.size)
    o = philox4x32_10((5, 0, 1, 0), (0x5EED0000, 0))
    u = [np.float32((int(v) >> 8) + 1) * np.float32(2.0 ** -24) for v in o]
    assert [bool(x > 0) for x in m.reshape(-1)[20:24]] == [bool(x > np.float32(0.4)) for x in u]
    assert not np.array_equal(m, dropout_mask(0x5EED0000, 2, 0, 64, 96, 0.4))
    assert not np.array_equal(m, dropout_mask(0x5EED0000, 1, 1, 64, 96, 0.4))
    # a width that is no multiple of 4: rows start inside a group, the index still decides
    m50 = dropout_mask(7, 0, 0, 3, 50, 0.1).reshape(-1)
    assert np.array_equal(m50[:148], dropout_mask(7, 0, 0, 37, 4, 0.1).reshape(-1))


# ---------------------------------------------------------------------------------------------
# masks unchanged on every path
# ---------------------------------------------------------------------------------------------
def _native():
    from lipasr import _native as N

    return N


def g(kind, exchange, amode, bmode, arith, epi):
    return (kind, exchange, amode, bmode, arith, epi)


def _exch(kind, a):
    return [g(kind, 1, 0, 1, a, EPI_BIAS_RELU_BNX), g(kind, 1, 0, 0, a, EPI_DH_BNX)]


W_ONE = (40, 96, 10)              # 3 column tiles of 32; batch 70 = two row tiles of 32 and 6 rows
W_MOD4 = (40, 50, 10)             # 50 columns: rows start at e = 50 r, every other one inside a group; the last group has 2 columns
W_TWO = (40, 96, 72, 10)          # 64 x 64 tiles: 96 = 64 + 32 and 72 = 64 + 8 columns, 70 = 64 + 6 rows; K = 40 / 96 / 72 >= 32
W_RING = (100, 136, 72, 70, 10)   # the shapes of test_gemm_instances_gpu.py's ring cases: layers 0 and 1 are ring-legal


def _case(id, widths, batch, rates, arith, claims, fuse=1, tiles=0, cus=0, knob=0, bn_off=()):
    return dict(id=id, widths=widths, batch=batch, rates=rates, arith=arith, claims=claims, fuse=fuse, tiles=tiles, cus=cus, knob=knob, bn_off=bn_off)


CASES = (
    # fragment exchange tiles, ragged rows; both rates of the classifier
    [_case(f"frag-exchange-r{r}-a{a}", W_ONE, 70, (r,), a, _exch(FRAG4, a)) for r in (0.4, 0.1) for a in (0, 2)]
    # ld = 50: nothing is aligned, every group takes the call per element
    + [_case(f"width-50-a{a}", W_MOD4, 70, (0.4,), a, _exch(FRAG4, a)) for a in (0, 2)]
    # no BatchNorm: dropout in bn_apply_fwd_kernel (forward) and EPI_DZ_NOBN (backward).  Mode 0 only: the library refuses mode 2
    # for a plan with a hidden layer without BatchNorm
    + [_case("no-batchnorm-a0", W_ONE, 70, (0.4,), 0, [g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU), g(FRAG4, 0, 0, 0, 0, EPI_DZ_NOBN)], bn_off=(0,))]
    # the launch chain: bn_apply_fwd_kernel (forward) and EPI_DH_STATS (backward), on fragment and on 64 x 64 tiles
    + [_case(f"chain-a{a}", W_ONE, 70, (0.4,), a, [g(FRAG4, 0, 0, 1, a, EPI_BIAS_RELU_STATS), g(FRAG4, 0, 0, 0, a, EPI_DH_STATS)], fuse=0) for a in (0, 2)]
    + [_case(f"chain-lds-a{a}", W_TWO, 70, (0.4, 0.1), a, [g(LDS, 0, 0, 1, a, EPI_BIAS_RELU_STATS), g(LDS, 0, 0, 0, a, EPI_DH_STATS)], fuse=0, tiles=1,
             knob=KNOB_NO_RING if a == 2 else 0) for a in (0, 2)]
    # the LDS-tiled exchange tile (mode 2: with the ring switched off, which would take these ring-legal layers)
    + [_case(f"lds-exchange-a{a}", W_TWO, 70, (0.4, 0.1), a, _exch(LDS, a) + [g(FRAG4, 1, 0, 0, a, EPI_DH_BNX)], tiles=1, knob=KNOB_NO_RING if a == 2 else 0)
       for a in (0, 2)]
    # mode 2: the loader-wavefront ring instance (whole device), the 64 x 64 ring exchange tile (without it), and on a share of 10 CUs
    # the 128 x 64 exchange tile at batch 300 = two row tiles of 128 and 44 rows (layer 1 stays on the loader-wavefront instance there)
    + [_case("ring-x1-a2", W_RING, 150, (0.4, 0.1, 0.1), 2, _exch(RING_X1, 2), tiles=1),
       _case("ring-a2", W_RING, 150, (0.4, 0.1, 0.1), 2, _exch(RING, 2), tiles=1, knob=KNOB_NO_X1),
       _case("ring2-a2", W_RING, 300, (0.4, 0.1, 0.1), 2, _exch(RING2, 2) + [g(RING_X1, 1, 0, 1, 2, EPI_BIAS_RELU_BNX)], tiles=1, cus=10)]
)

_open_models = []


@pytest.fixture(autouse=True)
def _default_knobs_and_closed_models():
    yield
    _native().lib.lipasr_debug_gemm_mode(0)
    while _open_models:
        _open_models.pop().close()


def _spec(case):
    w = case["widths"]
    n = len(w) - 1
    return [P.LayerSpec(w[i], w[i + 1], i < n - 1 and i not in case["bn_off"], case["rates"][i] if i < n - 1 else 0.0, True) for i in range(n)]


def _problem(case):
    spec = _spec(case)
    p = P.init_params(spec, seed=4, dtype=np.float32, nonneg_init=True)
    rng = np.random.default_rng(case["batch"] + len(spec))
    for l, s in enumerate(spec):
        p.b[l] = (0.1 * rng.standard_normal(s.n_out)).astype(np.float32)
        if s.bn:
            p.gamma[l] = (1 + 0.2 * rng.standard_normal(s.n_out)).astype(np.float32)
            p.beta[l] = (0.1 * rng.standard_normal(s.n_out)).astype(np.float32)
    x = rng.standard_normal((case["batch"], spec[0].n_in)).astype(np.float32)
    y = P.to_categorical(rng.integers(0, spec[-1].n_out, case["batch"]), spec[-1].n_out)
    return spec, p, x, y


def _snapshot(keys):
    lib = _native().lib
    return {k: lib.lipasr_debug_gemm_launches(*k) for k in keys}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _two_steps(case, spec, p, x, y, external):
    """Two training steps with Adam between them; returns ({name: bits}, the launch counters of the case's claims that moved)."""
    N = _native()
    assert case["cus"] <= torch.cuda.get_device_properties(0).multi_processor_count
    m = build_model(spec, max_batch=case["batch"], compute_dtype="float32")
    _open_models.append(m)
    N.check(N.lib.lipasr_mlp_set_compute(m._plan, case["arith"]))
    N.check(N.lib.lipasr_mlp_set_fuse_bn(m._plan, case["fuse"]))
    N.check(N.lib.lipasr_mlp_set_gemm_tiles(m._plan, case["tiles"]))
    N.check(N.lib.lipasr_mlp_set_cu_budget(m._plan, case["cus"]))
    N.check(N.lib.lipasr_debug_gemm_mode(case["knob"]))
    load_params(m, p)
    xt, yt = dev(x), dev(y)
    batch = case["batch"]
    out, moved = {}, {}
    for step in (0, 1):
        masks = None
        if external:
            masks = [dev(dropout_mask(m._dropout_seed, l, step, batch, s.n_out, s.dropout)) if s.dropout > 0 else None for l, s in enumerate(spec)]
        before = _snapshot(case["claims"])
        m.train_fwd_bwd(xt, yt, masks=masks)
        assert m.exchange_errors() == 0, "an exchange gave up"  # (synchronises)
        after = _snapshot(case["claims"])
        for k in after:
            moved[k] = moved.get(k, 0) + after[k] - before[k]
        assert int(m._step.item()) == step
        out[f"grads{step}"] = _bits(m._grads)
        out[f"loss_rows{step}"] = _bits(m._loss_rows[:batch])
        out[f"correct_rows{step}"] = _bits(m._correct_rows[:batch])
        out[f"bnstate{step}"] = _bits(m._bnstate)
        m.apply_adam()
        out[f"params{step}"] = _bits(m._params)
    return out, moved


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_philox_dropout_equals_the_restated_masks(cuda, case):
    """Mode 1 (the kernels draw) against mode 2 (the kernels read the restatement's masks), two steps, bit for bit."""
    spec, p, x, y = _problem(case)
    drawn, moved = _two_steps(case, spec, p, x, y, external=False)
    missing = [k for k in case["claims"] if moved.get(k, 0) < 2]
    assert not missing, "claimed but did not run in both steps: " + ", ".join(f"{KINDS[k[0]]} exchange {k[1]} BMODE {k[3]} arith {k[4]} epilogue {k[5]}" for k in missing)
    read, _ = _two_steps(case, spec, p, x, y, external=True)
    # the masks matter: a step without dropout gives other gradients (so equal bits below are not two runs that ignore them)
    assert np.isfinite(drawn["grads0"].view(np.float32)).all()
    differing = [name for name in drawn if not np.array_equal(drawn[name], read[name])]
    for name in differing:
        a, b = drawn[name].view(np.float32), read[name].view(np.float32)
        print(f"{case['id']} {name}: {np.count_nonzero(drawn[name] != read[name])} of {a.size} words differ, max |d| {np.abs(a.astype(np.float64) - b).max():.3e}")
    assert not differing, differing


@gpu
def test_dropout_changes_the_step(cuda):
    """The comparison above is decisive: the same step without dropout, and with the masks of another step, leaves other gradients."""
    case = CASES[0]
    spec, p, x, y = _problem(case)
    m = build_model(spec, max_batch=case["batch"], compute_dtype="float32")
    _open_models.append(m)
    load_params(m, p)
    xt, yt = dev(x), dev(y)
    m.train_fwd_bwd(xt, yt)
    with_drop = _bits(m._grads)
    m.train_fwd_bwd(xt, yt, dropout=False)
    assert not np.array_equal(with_drop, _bits(m._grads))
    wrong = [dev(dropout_mask(m._dropout_seed, 0, 1, case["batch"], spec[0].n_out, spec[0].dropout)), None]
    m.train_fwd_bwd(xt, yt, masks=wrong)
    assert not np.array_equal(with_drop, _bits(m._grads))


# ---------------------------------------------------------------------------------------------
# the "buffer free" signal in the Adam kernel
# ---------------------------------------------------------------------------------------------
@gpu
def test_adam_kernel_raises_the_buffer_free_counter(cuda, monkeypatch):
    """Ten eager pipeline steps at batch 64 with device flags: free[b] is raised by the Adam kernel
    (lipasr_mlp_adam_project_product_signal), no signal launch ends the step, the parameters equal those of the same steps with
    events (LIPASR_GPU_FLAGS=0) bit for bit, synchronize() raises nothing and the counters hold the last steps' indices."""
    from lipasr.pipeline import TrainPipeline
    from lipasr.synth import synth_clips

    N = _native()
    spec = P.vd_constrained_spec()
    p = P.init_params(spec, seed=9, dtype=np.float32, nonneg_init=True)
    waves, labels = synth_clips(128, seed=31)
    wt, yt = dev(waves), dev(P.to_categorical(labels, 10))
    results = {}
    for flags in ("1", "0"):
        monkeypatch.setenv("LIPASR_GPU_FLAGS", flags)
        m = build_model(spec, max_batch=64)
        _open_models.append(m)
        load_params(m, p)
        pipe = TrainPipeline(m, batch=64, rho=0.1, constraint="product", sync_inputs=False)
        signals = []
        real_signal = N.lib.lipasr_flag_signal
        monkeypatch.setattr(N.lib, "lipasr_flag_signal", lambda *a: (signals.append(a[2]), real_signal(*a))[1])
        try:
            assert (pipe._flags is not None) == (flags == "1") and pipe._adam_signal == (flags == "1") and not pipe.use_graph
            for i in range(10):
                s = 64 * (i % 2)
                pipe.step(wt[s:s + 64], yt[s:s + 64])
            pipe.synchronize()
            if flags == "1":
                assert signals == list(range(1, 11)), signals  # "features ready" once per step, nothing else
                assert pipe._flags.tolist() == [9, 10, 9, 10]  # ready[0], ready[1], free[0], free[1]
                assert int(pipe._flag_err[0]) == 0
            results[flags] = (_bits(m._params), _bits(m._bnstate), _bits(pipe.norms), int(m._step.item()))
        finally:
            monkeypatch.setattr(N.lib, "lipasr_flag_signal", real_signal)
            pipe.close()
    assert results["0"][3] == results["1"][3] == 10
    for a, b in zip(results["1"][:3], results["0"][:3]):
        assert np.array_equal(a, b)
