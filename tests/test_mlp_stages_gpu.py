"""The training step's own kernels stage by stage against float64, and proof of which kernels ran: adam_nonneg_kernel / step_inc_kernel
(csrc/optim.hip), bn_apply_fwd_kernel / bn_apply_bwd_kernel / part_reduce_kernel (csrc/mlp_train.hip) and the three softmax forms
(csrc/mlp_infer.hip), and the second copies of that arithmetic in the GEMM epilogues (EPI_BIAS_RELU_BNX / EPI_DH_BNX, EPI_BIAS_SOFTMAX_CE; csrc/gemm_device.h,
gemm_frag.hip).  In the manner of test_mfcc_instances_gpu.py:

  * memory: every array the test owns (params, grads, m, v, the step word, x, y, masks, the `part` buffer, every destination of
    lipasr_debug_mlp_stage) is a Buf: between sentinels, all of which must survive.  Plans have max_batch > batch; rows >= batch of a
    hook's destination still hold sentinels.
  * kernels: every case names the counters of lipasr_debug_k2_launches that must move and by how much; exactly those move (so
    bn_apply_* stays at zero on the exchange path and part_reduce_kernel outside segment mode).  Which GEMM epilogue ran instead is
    shown with lipasr_debug_gemm_launches.  The last test fails when the library knows a K2 id that no case claims and prints (-s)
    per kernel the first case that ran it and its worst error as a fraction of its bound.
  * determinism: every case runs twice into fresh buffers (and a fresh plan), bit for bit.
  * every tolerance is a bound tests/mlp_stage_ref.py computes from the inputs; test_mlp_stages_cpu.py shows that a float32
    restatement stays inside each and every mutant falls outside.
  * every case sets lipasr_mlp_set_fuse_bn, lipasr_mlp_set_compute (0: exact fp32) and lipasr_debug_gemm_mode (0) itself; the plan
    dies with the case and the global GEMM knob is put back to 0.

BatchNorm shapes: mlp_stage_ref.BN_SHAPES lists the condition each (N, B) is there for.  With these widths every GEMM takes the
32 x 32 fragment tile (asserted through the GEMM launch counters), so the column partial sums reach BatchNorm per 32 rows: B = 300
gives ten row tiles.  A statement through lipasr_mlp_adam_project_product: the product projection scales every VISITED kernel by
(rho / norm)^(1/m) whatever rho is -- it is never the identity for a visited layer -- so the comparison with lipasr_mlp_adam_nonneg
visits no layer (n_order = 0: the product norm is evaluated, the step word moves inside that kernel, no weight is scaled).

UNREACHABLE lists what no case can run.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_stage_ref as R
from test_dropout_quads_gpu import dropout_mask
from test_mfcc_instances_gpu import SENTINEL, Buf

pytestmark = pytest.mark.gpu

(BN_FWD, DROPOUT_FWD, BN_BWD, PART_REDUCE, SOFTMAX_CE, SOFTMAX_VJP, SOFTMAX_VJP_ONEHOT, ADAM, STEP_INC) = range(9)
K2_NAMES = ("bn_apply_fwd_kernel", "bn_apply_fwd_kernel (dropout only)", "bn_apply_bwd_kernel", "part_reduce_kernel", "softmax_ce_kernel",
            "softmax_vjp_kernel", "softmax_vjp_onehot_kernel", "adam_nonneg_kernel", "step_inc_kernel")
UNREACHABLE = {}  # what no case can run -> why (nothing today)
FRAG4 = 0
EPI_STATS, EPI_DH_STATS, EPI_DZ_NOBN, EPI_SOFTMAX_CE, EPI_BNX, EPI_DH_BNX = 6, 7, 8, 9, 10, 11
SEG_W, SEG_B, SEG_GAMMA, SEG_BETA, SEG_MMEAN, SEG_MVAR = range(6)

_ran = {}    # kernel id -> the first case whose counter assertion showed it running
_worst = {}  # kernel id -> (worst error as a fraction of its bound, the case, the quantity)


def _native():
    from lipasr import _native as N

    return N


def _snapshot():
    lib = _native().lib
    return [lib.lipasr_debug_k2_launches(k) for k in range(len(K2_NAMES))]


def _assert_moved(before, expect, what):
    moved = {k: a - b for k, (b, a) in enumerate(zip(before, _snapshot())) if a != b}
    names = lambda d: {K2_NAMES[k]: v for k, v in d.items()}
    assert moved == {k: v for k, v in expect.items() if v}, f"{what}: launched {names(moved)}, the case is meant to launch {names(expect)}"


def _gemm(*key):
    return _native().lib.lipasr_debug_gemm_launches(*key)


def _record(case_id, kernels, frac, what):
    for k in kernels:
        _ran.setdefault(k, case_id)
        if k not in _worst or frac > _worst[k][0]:
            _worst[k] = (frac, case_id, what)


def _frac(got, ref, bound):
    with np.errstate(all="ignore"):
        return float((np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / bound).max())


def _held(case_id, kernels, what, got, ref, bound):
    """asserts |got - ref| <= bound on every element; returns and records the worst fraction"""
    fr = _frac(got, ref, bound)
    print(f"{case_id}: {what} at {fr:.3f} of its bound")
    _record(case_id, kernels, fr, what)
    assert fr <= 1.0, f"{case_id}: {what} at {fr:.3g} of its bound"
    return fr


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(autouse=True)
def _default_knobs():
    _native().lib.lipasr_debug_gemm_mode(0)
    yield
    _native().lib.lipasr_debug_gemm_mode(0)


class Mlp:
    """A classifier plan through the raw C entry points, exact fp32, the fuse mode the case names."""

    def __init__(self, widths, bn, dropout, nonneg, max_batch, fuse=0):
        N = _native()
        self.widths, self.L, self.max_batch = tuple(widths), len(widths) - 1, max_batch
        self.h = N.c_h()
        N.check(N.lib.lipasr_mlp_create(N.get_handle(0).h, self.L, N.int_array(widths), N.int_array(bn), N.float_array(dropout),
                                        N.int_array(nonneg), max_batch, C.byref(self.h)))
        N.check(N.lib.lipasr_mlp_set_fuse_bn(self.h, fuse))
        N.check(N.lib.lipasr_mlp_set_compute(self.h, 0))
        N.check(N.lib.lipasr_debug_gemm_mode(0))
        a, b = N.sz(), N.sz()
        N.check(N.lib.lipasr_mlp_sizes(self.h, C.byref(a), C.byref(b)))
        self.n_params, self.n_state = a.value, b.value

    def seg(self, layer, kind):
        N = _native()
        o, c = N.sz(), N.sz()
        N.check(N.lib.lipasr_mlp_segment(self.h, layer, kind, C.byref(o), C.byref(c)))
        return o.value, c.value

    def flat(self, tensors, state=False):
        """{(layer, kind): array} -> the flat float32 buffer (zeros on the padding)"""
        out = np.zeros(self.n_state if state else self.n_params, np.float32)
        for (l, kind), a in tensors.items():
            o, c = self.seg(l, kind)
            assert c == np.size(a)
            out[o:o + c] = np.asarray(a, np.float32).ravel()
        return out

    def stage(self, layer, which, batch):
        """lipasr_debug_mlp_stage into a guarded destination laid out for max_batch rows"""
        N = _native()
        n = self.widths[layer + 1]
        dst = Buf((2, n)) if which == 2 else Buf((self.max_batch, n))
        N.check(N.lib.lipasr_debug_mlp_stage(self.h, layer, which, batch, dst.ptr(), N.stream_ptr()))
        torch.cuda.synchronize()
        return dst.read() if which == 2 else dst.read(batch)

    def errors(self):
        N = _native()
        e = C.c_int()
        N.check(N.lib.lipasr_mlp_exchange_errors(self.h, C.byref(e)))
        return e.value

    def close(self):
        if self.h:
            N = _native()
            torch.cuda.synchronize()
            N.check(N.lib.lipasr_mlp_destroy(self.h))
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _twice(run):
    """run() twice (fresh plan, fresh buffers each time) -> the first result; every array of the two results has the same bits"""
    a, b = run(), run()
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert _same(a[k], b[k]), f"{k}: two runs from the same inputs differ"
    return a


# ====================================================================================================== the layout and the hooks
def test_segments_restatement_is_the_plans_layout(cuda):
    for widths, bn, nonneg in (((5, 7, 3), (1, 0), (1, 0)), ((1500, 1500, 10), (0, 0), (1, 1)), ((6, 33, 3), (1, 0), (0, 0))):
        segs, n = R.segments(widths, bn, nonneg)
        with Mlp(widths, bn, (0, 0), nonneg, 4) as plan:
            assert plan.n_params == n
            kinds = {"W": SEG_W, "b": SEG_B, "gamma": SEG_GAMMA, "beta": SEG_BETA}
            for name, l, start, count, _ in segs:
                assert plan.seg(l, kinds[name]) == (start, count)


def test_stage_hook_refuses_what_a_layer_does_not_have(cuda):
    """Every (layer, which) of a three-layer plan after one inference forward of 3 rows: what the layer has is copied (rows >= 3 of the
    destination keep their sentinels, the logits are the ones lipasr_mlp_predict returns, bit for bit), everything else is refused
    and writes nothing.  Twice, bit for bit."""
    N = _native()
    ok = [(0, w) for w in (0, 1, 2, 3, 4)] + [(1, 0), (1, 1), (1, 3), (2, 3), (2, 5), (2, 6)]
    bad = [(0, 5), (0, 6), (1, 2), (1, 4), (2, 0), (2, 1), (2, 2), (2, 4), (0, 7), (0, -1), (3, 0), (-1, 0)]

    def run():
        out = {}
        with Mlp((6, 8, 8, 3), (1, 0, 0), (0, 0, 0), (0, 0, 0), 4) as plan:
            params = Buf((plan.n_params,), 0.4 * np.random.default_rng(3).standard_normal(plan.n_params))
            state = Buf((plan.n_state,), np.ones(plan.n_state))
            x, logits = Buf((3, 6), np.random.default_rng(4).standard_normal((3, 6))), Buf((3, 3))
            before = _snapshot()
            N.check(N.lib.lipasr_mlp_predict(plan.h, params.ptr(), state.ptr(), x.ptr(), 3, None, logits.ptr(), N.stream_ptr()))
            _assert_moved(before, {}, "predict without probabilities")
            torch.cuda.synchronize()
            out["logits_caller"] = logits.read()
            own = Buf((3, 3))
            N.check(N.lib.lipasr_mlp_own_labels(plan.h, params.ptr(), state.ptr(), x.ptr(), 3, own.ptr(), N.stream_ptr()))  # logits into the plan
            for layer, which in ok:
                out[f"stage{layer}{which}"] = plan.stage(layer, which, 3)
            own.read()
            dst = Buf((4, 8))
            for layer, which in bad:
                assert N.lib.lipasr_debug_mlp_stage(plan.h, layer, which, 3, dst.ptr(), N.stream_ptr()) == N.EINVAL, (layer, which)
            for batch in (0, 5):
                assert N.lib.lipasr_debug_mlp_stage(plan.h, 0, 0, batch, dst.ptr(), N.stream_ptr()) == N.EINVAL
            assert N.lib.lipasr_debug_mlp_stage(plan.h, 0, 0, 4, None, N.stream_ptr()) == N.EINVAL
            assert N.lib.lipasr_debug_mlp_stage(None, 0, 0, 4, dst.ptr(), N.stream_ptr()) == N.EINVAL
            torch.cuda.synchronize()
            assert (dst.read() == np.float32(SENTINEL)).all(), "a refused call wrote"
            for b in (params, state, x):
                b.read()
        return out

    o = _twice(run)
    assert _same(o["stage25"], o["logits_caller"]), "hook 5 is not the logits"
    assert np.abs(o["stage01"]).max() > 0 and _same(o["stage10"], o["stage11"]), "H_1 aliases A_1 on a layer without BatchNorm and dropout"


def test_create_refuses_33_classes(cuda):
    N = _native()
    h = N.c_h()
    rc = N.lib.lipasr_mlp_create(N.get_handle(0).h, 1, N.int_array((33, 33)), N.int_array((0,)), N.float_array((0,)), N.int_array((0,)), 4, C.byref(h))
    assert rc == N.EINVAL and "at most 32" in N.last_error()


# ====================================================================================================== K5 Adam + NonNeg
ADAM_MODELS = R.ADAM_MODELS  # the CPU companion puts the same plans, inputs and (t, gscale) through the float32 restatement
ADAM_CASES = ([(m, t, R.ADAM_GSCALE) for m in ("nonneg-layer-0", "nonneg-layer-1") for t in R.ADAM_T]
              + [("stride-loop", t, (gs,)) for t, gs in R.ADAM_STRIDE_LOOP_CASES])


def _adam_call(plan, arrays, t_word, gscale, product=False):
    N = _native()
    hp = R.ADAM_HP
    w, g, m, v = (Buf(a.shape, a) for a in arrays)
    step = Buf((1,), [t_word], dtype=np.int32)
    args = (plan.h, w.ptr(), g.ptr(), m.ptr(), v.ptr(), step.ptr(), hp["lr"], hp["b1"], hp["b2"], hp["eps"], gscale)
    out = {}
    if product:
        norms = Buf((1,))
        N.check(N.lib.lipasr_mlp_adam_project_product(*args, 1e6, None, 0, norms.ptr(), N.stream_ptr()))
    else:
        N.check(N.lib.lipasr_mlp_adam_nonneg(*args, N.stream_ptr()))
    torch.cuda.synchronize()
    if product:
        out["norm"] = norms.read()
    out.update(w=w.read(), m=m.read(), v=v.read(), step=step.read())
    assert _same(g.read(), arrays[1]), "the gradients were written"
    return out


@pytest.mark.parametrize("model,t_word,gscales", ADAM_CASES, ids=[f"{m}-t{t}" for m, t, _ in ADAM_CASES])
def test_adam_nonneg(cuda, model, t_word, gscales):
    widths, bn, nonneg = ADAM_MODELS[model]
    segs, n = R.segments(widths, bn, nonneg)
    assert model != "stride-loop" or (n >> 2) > 2048 * 256
    arrays = R.adam_inputs(segs, n, R.ADAM_SEED)
    clamp, live = R.clamp_mask(segs, n), R.live_mask(segs, n)
    for gscale in gscales:
        case = f"adam-{model}-t{t_word}-g{gscale:.3f}"

        def run(product=False):
            with Mlp(widths, bn, (0, 0), nonneg, 4) as plan:
                assert plan.n_params == n
                before = _snapshot()
                out = _adam_call(plan, arrays, t_word, gscale, product)
                _assert_moved(before, {ADAM: 1, STEP_INC: 0 if product else 1}, case)
            return out

        got = _twice(run)
        assert got["step"][0] == t_word + 1
        ref = R.adam(*arrays, t_word, gscale=gscale, clamp=clamp, **R.ADAM_HP)
        for k, b in (("w", "bw"), ("m", "bm"), ("v", "bv")):
            _held(case, (ADAM,), k, got[k], ref[k], ref[b])
            assert (got[k][~live] == 0).all(), "a padding float (zero in) is not zero out"
        _record(case, (STEP_INC,), 0.0, "step word")
        w0 = arrays[0]
        for name, l, s, c, cl in segs:
            if c < 6:
                continue
            assert _same(got["w"][s:s + 1], w0[s:s + 1]), "g = m = v = 0 moved a weight"
            assert got["w"][s + 1] == 0 and not np.signbit(got["w"][s + 1]) and got["w"][s + 2] == 0 and np.signbit(got["w"][s + 2])
            # the update drives this weight negative: NonNeg gives exactly +0.0, any other segment keeps the negative value
            assert (_same(got["w"][s + 3:s + 4], np.zeros(1, np.float32))) if cl else (got["w"][s + 3] < 0), (name, l)
        if model != "stride-loop":
            # the same inputs through the fused entry point, no layer visited: same w, m, v, the step word moved inside the
            # projection's kernel, step_inc_kernel did not run (asserted in run)
            fused = _twice(lambda: run(product=True))
            assert fused["step"][0] == t_word + 1 and np.isfinite(fused["norm"]).all() and fused["norm"][0] > 0
            for k in ("w", "m", "v"):
                assert _same(fused[k], got[k]), f"lipasr_mlp_adam_project_product: {k} differs from lipasr_mlp_adam_nonneg"


def test_adam_non_finite_gradients_poison_the_weight(cuda):
    """A NaN and an inf gradient in a NonNeg segment and in the others: m and v come out non-finite, and so does w -- Keras' NonNeg is
    w (w >= 0), which keeps a NaN; the kernel wrote 0 there (`!(x >= 0) ? 0 : x`) until this suite, with no reason on record, so a
    poisoned step left healthy-looking weights.  Every other element is held to its bound as usual."""
    widths, bn, nonneg = ADAM_MODELS["nonneg-layer-0"]
    segs, n = R.segments(widths, bn, nonneg)
    arrays = R.adam_inputs(segs, n, R.ADAM_SEED, nonfinite=True)
    clamp = R.clamp_mask(segs, n)

    def run():
        with Mlp(widths, bn, (0, 0), nonneg, 4) as plan:
            before = _snapshot()
            out = _adam_call(plan, arrays, 0, 1.0)
            _assert_moved(before, {ADAM: 1, STEP_INC: 1}, "adam-non-finite")
        return out

    got = _twice(run)  # (the bits of the NaNs included)
    ref = R.adam(*arrays, 0, gscale=1.0, clamp=clamp, **R.ADAM_HP)
    poisoned = np.zeros(n, bool)
    for name, l, s, c, cl in segs:
        if c >= 6:
            poisoned[s + 4:s + 6] = True
            for k in ("m", "v"):
                assert not np.isfinite(got[k][s + 4:s + 6]).any(), (name, l, k)
            assert np.isnan(got["w"][s + 4:s + 6]).all(), (name, l, "a poisoned update left a finite weight")
    assert poisoned.sum() == 10 and np.isnan(ref["w"][poisoned]).all()
    for k, b in (("w", "bw"), ("m", "bm"), ("v", "bv")):
        _held("adam-non-finite", (ADAM,), k, got[k][~poisoned], ref[k][~poisoned], ref[b][~poisoned])


# ====================================================================================================== BatchNorm / dropout apply
def _train_call(plan, mdl, B, cfg, with_probs=False, seg=None, part=None, stat_batch=0, grad_scale=1.0, inv_batch=None, bufs=None):
    """one lipasr_mlp_train_fwd_bwd (or one segment of lipasr_mlp_train_segment) on fresh guarded buffers -> the buffers"""
    N = _native()
    C_ = plan.widths[-1]
    if bufs is None:
        tensors = {(0, SEG_W): mdl["W0"], (0, SEG_B): mdl["b0"], (1, SEG_W): mdl["W1"], (1, SEG_B): mdl["b1"]}
        state = {}
        if plan.n_state:
            tensors.update({(0, SEG_GAMMA): mdl["gamma"], (0, SEG_BETA): mdl["beta"]})
            state = {(0, SEG_MMEAN): mdl["mmean"], (0, SEG_MVAR): mdl["mvar"]}
        bufs = dict(params=Buf((plan.n_params,), plan.flat(tensors)), bnstate=Buf((max(plan.n_state, 1),), plan.flat(state, True) if plan.n_state else None),
                    x=Buf(mdl["x"].shape, mdl["x"]), y=Buf(mdl["y"].shape, mdl["y"]), grads=Buf((plan.n_params,)), loss=Buf((B,)),
                    correct=Buf((B,)), probs=Buf((B, C_)) if with_probs else None)
    b = bufs
    common = (b["params"].ptr(), b["bnstate"].ptr(), b["x"].ptr(), b["y"].ptr(), B, 1.0 / B if inv_batch is None else inv_batch, C.byref(cfg),
              b["grads"].ptr(), b["loss"].ptr(), b["correct"].ptr(), b["probs"].ptr() if b["probs"] is not None else None)
    if seg is None:
        N.check(N.lib.lipasr_mlp_train_fwd_bwd(plan.h, *common, N.stream_ptr()))
    else:
        N.check(N.lib.lipasr_mlp_train_segment(plan.h, seg, *common, part.ptr(), stat_batch, grad_scale, N.stream_ptr()))
    torch.cuda.synchronize()
    return bufs


def _mask_cfg(mask_buf):
    N = _native()
    cfg = N.DropoutCfg()
    if mask_buf is None:
        cfg.mode = 0
        return cfg, None
    cfg.mode = 2
    ptrs = N.ptr_array([mask_buf.ptr().value, None])
    cfg.masks = C.cast(ptrs, N.PV)
    return cfg, ptrs


BN_CASES = ([(N_, B, path, "masks") for (N_, B) in R.BN_SHAPES for path in ("chain", "exchange")]
            + [(33, 33, "chain", "philox"), (33, 33, "exchange", "philox")])
PHILOX_SEED, PHILOX_STEP = 0x5EED0007, 3


def _bn_check(case, kernels, mdl, mask, B, N_, A, H, stats, state, dz0, g, dg, grads_dbeta, grads_dgamma, Bstat=None, extra=0, grad_scale=1.0,
              A_all=None, g_all=None, dg_all=None):
    """the per-stage statements of one plan's BatchNorm layer; *_all: the stacked shards under synchronized BatchNorm"""
    fwd, bwd = kernels
    A_all = A if A_all is None else A_all
    st = R.bn_stats(A_all, mdl["mmean"], mdl["mvar"], Bstat=Bstat, extra=extra)
    mean, rstd = stats[0], stats[1]
    _held(case, fwd, "mean", mean, st["mean"], st["b_mean"])
    _held(case, fwd, "rstd", rstd, st["rstd"], st["b_rstd"])
    _held(case, fwd, "moving mean", state[0], st["mmean"], st["b_mmean"])
    _held(case, fwd, "moving variance", state[1], st["mvar"], st["b_mvar"])
    if N_ > 2 and A_all.shape[0] >= 7:
        print(f"{case}: offset unit (mean / std {A_all[:, 2].mean() / A_all[:, 2].std():.0f}): rstd {rstd[2]:.6g}, error {abs(rstd[2] - st['rstd'][2]):.3g}, "
              f"bound {st['b_rstd'][2]:.3g} ({st['b_rstd'][2] / st['rstd'][2]:.2e} of rstd)")
    Href, bH = R.bn_apply(A, mean, rstd, mdl["gamma"], mdl["beta"], mask)
    _held(case, fwd, "H", H, Href, bH)
    if mask is not None:
        assert (H[mask == 0] == 0).all() and ((mask == 0).any() or mask.size < 16)
    g_all, dg_all = (g if g_all is None else g_all), (dg if dg_all is None else dg_all)
    db, dgm, bdb, bdg = R.bn_bwd_sums(g_all, A_all, mean, rstd, extra=extra, dg=dg_all)
    dev_db, dev_dg = grads_dbeta / np.float32(grad_scale), grads_dgamma / np.float32(grad_scale)  # (a power of two: exact)
    _held(case, bwd, "dbeta", dev_db, db, bdb)
    _held(case, bwd, "dgamma", dev_dg, dgm, bdg)
    dz, bdz = R.bn_bwd_dz(g, A, mean, rstd, mdl["gamma"], dev_db, dev_dg, Bstat or B, dg=dg)
    live = A > 0
    assert (dz0[~live] == 0).all(), "dz is not exactly 0 where a <= 0"
    _held(case, bwd, "dz", dz0[live], dz[live], bdz[live])
    assert (A[:, 0] == 0).all() and (dz0[:, 0] == 0).all()  # the dead unit
    if N_ > 1:
        assert (A[:, 1] == np.float32(0.75)).all() and mean[1] == np.float32(0.75)  # the constant unit: zero variance
        np.testing.assert_allclose(rstd[1], 1 / np.sqrt(R.BN_EPS), rtol=1e-6)


@pytest.mark.parametrize("N_,B,path,drop", BN_CASES, ids=[f"N{n}-B{b}-{p}-{d}" for n, b, p, d in BN_CASES])
def test_batchnorm_apply_stages(cuda, N_, B, path, drop):
    N = _native()
    case = f"bn-N{N_}-B{B}-{path}-{drop}"
    mdl = R.bn_model(R.BN_N_IN, N_, R.BN_C, B)
    fuse = 1 if path == "exchange" else 0
    if drop == "masks":
        mask = R.dropout_masks(B, N_, R.BN_RATE, N_ + B)
    else:
        mask = dropout_mask(PHILOX_SEED, 0, PHILOX_STEP, B, N_, R.BN_RATE)
    gk_f = (FRAG4, fuse, 0, 1, 0, EPI_BNX if fuse else EPI_STATS)
    gk_b = (FRAG4, fuse, 0, 0, 0, EPI_DH_BNX if fuse else EPI_DH_STATS)
    expect = {} if fuse else {BN_FWD: 1, BN_BWD: 1}

    def run():
        with Mlp((R.BN_N_IN, N_, R.BN_C), (1, 0), (R.BN_RATE, 0), (0, 0), B + 5, fuse=fuse) as plan:
            pf = N.sz()
            N.check(N.lib.lipasr_mlp_part_floats(plan.h, C.byref(pf)))
            assert pf.value == 2 * ((B + 5 + 31) // 32) * max(plan.widths)  # one [2][N] slab per 32-row tile
            if drop == "masks":
                mb = Buf(mask.shape, mask)
                cfg, keep = _mask_cfg(mb)
            else:
                mb = Buf((1,), [PHILOX_STEP], dtype=np.int32)
                cfg = N.DropoutCfg()
                cfg.mode, cfg.seed, cfg.step_dev = 1, PHILOX_SEED, mb.ptr().value
            before, gf, gb = _snapshot(), _gemm(*gk_f), _gemm(*gk_b)
            b = _train_call(plan, mdl, B, cfg)
            _assert_moved(before, expect, case)
            assert _gemm(*gk_f) == gf + 1 and _gemm(*gk_b) == gb + 1, "the GEMMs did not take the 32 x 32 fragment tile with the epilogue the case names"
            assert plan.errors() == 0
            mb.read()
            out = dict(A=plan.stage(0, 0, B), H=plan.stage(0, 1, B), stats=plan.stage(0, 2, B), dz0=plan.stage(0, 3, B), dz1=plan.stage(1, 3, B),
                       g=plan.stage(0, 4, B), grads=b["grads"].read(), state=b["bnstate"].read(), loss=b["loss"].read(), correct=b["correct"].read())
            for k in ("params", "x", "y"):
                b[k].read()
            out["og"], out["obe"] = plan.seg(0, SEG_GAMMA)[0], plan.seg(0, SEG_BETA)[0]
            out["omm"], out["omv"] = plan.seg(0, SEG_MMEAN)[0], plan.seg(0, SEG_MVAR)[0]
        return out

    o = _twice(run)
    if fuse:
        g, dg = R.g_from_next_layer(o["dz1"], mdl["W1"], mask)  # never in memory on this path
    else:
        g, dg = o["g"], None
    kernels = ((), ()) if fuse else ((BN_FWD,), (BN_BWD,))
    _bn_check(case, kernels, mdl, mask, B, N_, o["A"], o["H"], o["stats"], (o["state"][o["omm"]:o["omm"] + N_], o["state"][o["omv"]:o["omv"] + N_]),
              o["dz0"], g, dg, o["grads"][o["obe"]:o["obe"] + N_], o["grads"][o["og"]:o["og"] + N_])
    for k in kernels[0] + kernels[1]:
        _ran.setdefault(k, case)


def test_dropout_only_apply(cuda):
    """a layer with dropout and no BatchNorm: bn_apply_fwd_kernel with has_bn == 0 (counter id 1), H = a mask with one rounding"""
    N = _native()
    N_, B = 33, 33
    case = "dropout-only-N33-B33"
    mdl = R.bn_model(R.BN_N_IN, N_, R.BN_C, B)
    mask = R.dropout_masks(B, N_, R.BN_RATE, 5)

    def run():
        with Mlp((R.BN_N_IN, N_, R.BN_C), (0, 0), (R.BN_RATE, 0), (0, 0), B + 5) as plan:
            mb = Buf(mask.shape, mask)
            cfg, keep = _mask_cfg(mb)
            before, gb = _snapshot(), _gemm(FRAG4, 0, 0, 0, 0, EPI_DZ_NOBN)
            b = _train_call(plan, mdl, B, cfg)
            _assert_moved(before, {DROPOUT_FWD: 1}, case)
            assert _gemm(FRAG4, 0, 0, 0, 0, EPI_DZ_NOBN) == gb + 1
            mb.read()
            for k in ("params", "bnstate", "x", "y"):
                b[k].read()
            return dict(A=plan.stage(0, 0, B), H=plan.stage(0, 1, B), dz0=plan.stage(0, 3, B), dz1=plan.stage(1, 3, B), grads=b["grads"].read(),
                        loss=b["loss"].read(), correct=b["correct"].read())

    o = _twice(run)
    one, zero = np.ones(N_, np.float32), np.zeros(N_, np.float32)
    Href, bH = R.bn_apply(o["A"], zero, one, one, zero, mask)
    _held(case, (DROPOUT_FWD,), "H", o["H"], Href, bH)
    assert (o["H"][mask == 0] == 0).all()
    g, dg = R.g_from_next_layer(o["dz1"], mdl["W1"], mask)
    live = o["A"] > 0
    assert (o["dz0"][~live] == 0).all()
    _held(case, (), "dz (EPI_DZ_NOBN)", o["dz0"][live], g[live], dg[live])


# ====================================================================================================== synchronized BatchNorm, one process
def test_synchronized_batchnorm_two_plans_one_process(cuda):
    """A 64-row batch cut into 40 and 24 rows on two plans with the same parameters, run segment by segment (stat_batch 64,
    grad_scale 0.5).  Between segments the test adds the two caller-owned `part` buffers (one fp32 addition per float) and writes
    the sum to both: what the all-reduce does, with no process group.  40 rows are two 32-row tiles on one plan, 24 rows one tile on
    the other; part_reduce_kernel leaves [2][N] on each whatever the tile count."""
    N = _native()
    N_, B, cut = 33, 64, 40
    case = "syncbn-N33-40+24"
    mdl = R.bn_model(R.BN_N_IN, N_, R.BN_C, B)
    mask = R.dropout_masks(B, N_, R.BN_RATE, 64)
    rows = (slice(0, cut), slice(cut, B))

    def run():
        plans = [Mlp((R.BN_N_IN, N_, R.BN_C), (1, 0), (R.BN_RATE, 0), (0, 0), cut + 3) for _ in rows]
        try:
            ns = C.c_int()
            N.check(N.lib.lipasr_mlp_train_segments(plans[0].h, C.byref(ns)))
            assert ns.value == 3
            pf = N.sz()
            N.check(N.lib.lipasr_mlp_part_floats(plans[0].h, C.byref(pf)))
            parts = [Buf((pf.value,)) for _ in rows]
            shard = [dict(mdl, x=mdl["x"][r], y=mdl["y"][r]) for r in rows]
            mbs = [Buf(mask[r].shape, mask[r]) for r in rows]
            cfgs = [_mask_cfg(mb) for mb in mbs]
            bufs = [None, None]
            before = _snapshot()
            for seg in range(3):
                for i, r in enumerate(rows):
                    nb = r.stop - r.start
                    k2 = _snapshot()
                    bufs[i] = _train_call(plans[i], shard[i], nb, cfgs[i][0], seg=seg, part=parts[i], stat_batch=B, grad_scale=0.5, inv_batch=1.0 / B, bufs=bufs[i])
                    _assert_moved(k2, [{PART_REDUCE: 1}, {BN_FWD: 1, PART_REDUCE: 1}, {BN_BWD: 1}][seg], f"{case} segment {seg} plan {i}")
                ex = N.sz()
                N.check(N.lib.lipasr_mlp_train_segment_exchange(plans[0].h, cut, seg, C.byref(ex)))
                assert ex.value == (2 * N_ if seg < 2 else 0)
                if ex.value:
                    # the n_tiles part_reduce_kernel was given, read off what it left: the GEMM wrote [2][n_tiles][N] and the
                    # reduction overwrote the first [2][N], so with two row tiles the two tiles of the second statistic are still
                    # behind it (and add up, in fp64, to the reduced value), with one tile nothing was ever written there
                    for i, tiles in enumerate((2, 1)):
                        ph = parts[i].read()
                        tail = ph[2 * N_:2 * tiles * N_] if tiles > 1 else ph[:0]
                        assert (ph[2 * tiles * N_:] == np.float32(SENTINEL)).all() and (tail != np.float32(SENTINEL)).all(), \
                            f"{case} segment {seg} plan {i}: the partial sums are not those of {tiles} row tile(s)"
                        if tiles > 1:
                            both = (tail[:N_].astype(np.float64) + tail[N_:]).astype(np.float32)
                            assert _same(both, ph[N_:2 * N_]), "part_reduce_kernel: not the fp64 sum of the two tiles"
                        parts[i].t[parts[i].start + 2 * N_:parts[i].start + parts[i].n] = SENTINEL
                    views = [p.t[p.start:p.start + ex.value] for p in parts]
                    total = views[0] + views[1]
                    for v in views:
                        v.copy_(total)
                    torch.cuda.synchronize()
            _assert_moved(before, {PART_REDUCE: 4, BN_FWD: 2, BN_BWD: 2}, case)
            out = {}
            for i, r in enumerate(rows):
                nb = r.stop - r.start
                p = plans[i]
                for name, (l, w) in dict(A=(0, 0), H=(0, 1), stats=(0, 2), dz0=(0, 3), g=(0, 4)).items():
                    out[f"{name}{i}"] = p.stage(l, w, nb)
                out[f"grads{i}"], out[f"state{i}"] = bufs[i]["grads"].read(), bufs[i]["bnstate"].read()
                parts[i].read(); mbs[i].read()
                for k in ("params", "x", "y", "loss", "correct"):
                    bufs[i][k].read()
            out["off"] = np.array([plans[0].seg(0, k)[0] for k in (SEG_GAMMA, SEG_BETA, SEG_MMEAN, SEG_MVAR)])
        finally:
            for p in plans:
                p.close()
        return out

    o = _twice(run)
    og, obe, omm, omv = (int(v) for v in o["off"])
    assert _same(o["stats0"], o["stats1"]) and _same(o["state0"], o["state1"]), "the two plans hold different statistics"
    for k in (og, obe):
        assert _same(o["grads0"][k:k + N_], o["grads1"][k:k + N_]), "both plans scale the same global sums"
    A_all, g_all = np.concatenate([o["A0"], o["A1"]]), np.concatenate([o["g0"], o["g1"]])
    for i, r in enumerate(rows):
        _bn_check(f"{case} plan {i}", ((BN_FWD, PART_REDUCE), (BN_BWD, PART_REDUCE)), mdl, mask[r], r.stop - r.start, N_, o[f"A{i}"], o[f"H{i}"], o[f"stats{i}"],
                  (o[f"state{i}"][omm:omm + N_], o[f"state{i}"][omv:omv + N_]), o[f"dz0{i}"], o[f"g{i}"], None, o[f"grads{i}"][obe:obe + N_],
                  o[f"grads{i}"][og:og + N_], Bstat=B, extra=2, grad_scale=0.5, A_all=A_all, g_all=g_all)
    # the gradient all-reduce sums the two plans' values: the 64-row sums
    db, dgm, bdb, bdg = R.bn_bwd_sums(g_all, A_all, o["stats0"][0], o["stats0"][1], extra=3)
    _held(case, (BN_BWD,), "dbeta of both plans", o["grads0"][obe:obe + N_].astype(np.float64) + o["grads1"][obe:obe + N_], db, bdb)
    _held(case, (BN_BWD,), "dgamma of both plans", o["grads0"][og:og + N_].astype(np.float64) + o["grads1"][og:og + N_], dgm, bdg)


def test_segments_of_a_plan_with_two_batchnorm_layers_out_of_three(cuda):
    """Widths (5, 9, 33, 7, 3), BatchNorm on the second and third hidden layer only, no dropout, 7 rows on a plan for 10: the exchange
    points are forward layer 1 (33 wide), forward layer 2 (7), backward layer 2, backward layer 1 -- five segments, 66, 14, 14, 66
    floats to exchange and none after the last.  The five segments in order on one plan (caller-owned `part`, stat_batch 7,
    grad_scale 1, nothing between them: one rank's sum is itself) against ONE lipasr_mlp_train_fwd_bwd on the launch chain of a second,
    identical plan: the same bits everywhere.  Seven rows are one row tile, part_reduce_kernel over one tile stores (float)(double)x,
    and the apply kernels read one tile on both paths."""
    N = _native()
    widths, bn, B, max_batch = (5, 9, 33, 7, 3), (0, 1, 1, 0), 7, 10
    rng = np.random.default_rng(20251)
    tensors, state = {}, {}
    for l in range(4):
        tensors[(l, SEG_W)] = 0.4 * rng.standard_normal((widths[l], widths[l + 1]))
        tensors[(l, SEG_B)] = 0.1 * rng.standard_normal(widths[l + 1])
        if bn[l]:
            tensors[(l, SEG_GAMMA)] = 1.0 + 0.1 * rng.standard_normal(widths[l + 1])
            tensors[(l, SEG_BETA)] = 0.1 * rng.standard_normal(widths[l + 1])
            state[(l, SEG_MMEAN)] = 0.1 * rng.standard_normal(widths[l + 1])
            state[(l, SEG_MVAR)] = 1.0 + 0.5 * rng.random(widths[l + 1])
    x = rng.standard_normal((B, widths[0])).astype(np.float32)
    y = np.eye(widths[-1], dtype=np.float32)[rng.integers(0, widths[-1], B)]
    stages = [(l, w) for l in range(3) for w in (0, 1, 3)] + [(1, 2), (2, 2), (3, 3)]

    def run():
        out = {}
        for name in ("segments", "chain"):
            with Mlp(widths, bn, (0, 0, 0, 0), (0, 0, 0, 0), max_batch, fuse=0) as plan:
                bufs = dict(params=Buf((plan.n_params,), plan.flat(tensors)), bnstate=Buf((plan.n_state,), plan.flat(state, True)), x=Buf(x.shape, x),
                            y=Buf(y.shape, y), grads=Buf((plan.n_params,)), loss=Buf((B,)), correct=Buf((B,)), probs=None)
                cfg = N.DropoutCfg()
                cfg.mode = 0
                before = _snapshot()
                if name == "segments":
                    ns, pf, ex = C.c_int(), N.sz(), N.sz()
                    N.check(N.lib.lipasr_mlp_train_segments(plan.h, C.byref(ns)))
                    assert ns.value == 5
                    sizes = []
                    for seg in range(5):
                        N.check(N.lib.lipasr_mlp_train_segment_exchange(plan.h, B, seg, C.byref(ex)))
                        sizes.append(ex.value)
                    assert sizes == [66, 14, 14, 66, 0]
                    N.check(N.lib.lipasr_mlp_part_floats(plan.h, C.byref(pf)))
                    part = Buf((pf.value,))
                    for seg in range(5):
                        _train_call(plan, None, B, cfg, seg=seg, part=part, stat_batch=B, grad_scale=1.0, bufs=bufs)
                    _assert_moved(before, {PART_REDUCE: 4, BN_FWD: 2, BN_BWD: 2}, "two-of-three segments")
                    part.read()
                else:
                    _train_call(plan, None, B, cfg, bufs=bufs)
                    _assert_moved(before, {BN_FWD: 2, BN_BWD: 2}, "two-of-three chain")
                assert plan.errors() == 0
                for l, w in stages:
                    out[f"{name}-stage{l}{w}"] = plan.stage(l, w, B)
                for k, b in (("grads", "grads"), ("state", "bnstate"), ("loss", "loss"), ("correct", "correct")):
                    out[f"{name}-{k}"] = bufs[b].read()
                for k in ("params", "x", "y"):
                    bufs[k].read()
        return out

    o = _twice(run)
    for k in [k[len("chain-"):] for k in o if k.startswith("chain-")]:
        assert _same(o[f"segments-{k}"], o[f"chain-{k}"]), f"{k}: the five segments and the one call differ"
    assert np.isfinite(o["chain-grads"]).all() and np.abs(o["chain-stage03"]).max() > 0 and np.isfinite(o["chain-loss"]).all()
    _record("two-of-three segments", (PART_REDUCE,), 0.0, "same bits as the launch chain")


# ====================================================================================================== softmax
SOFTMAX_CASES =[(C_, B) for C_ in (1, 2, 10, 32) for B in (1, 255, 257)]


def _identity(plan, C_):
    return Buf((plan.n_params,), plan.flat({(0, SEG_W): np.eye(C_, dtype=np.float32), (0, SEG_B): np.zeros(C_, np.float32)}))


@pytest.mark.parametrize("C_,B", SOFTMAX_CASES, ids=[f"C{c}-B{b}" for c, b in SOFTMAX_CASES])
def test_softmax_forms(cuda, C_, B):
    """One-layer plans (C, C) with W = I, b = 0: the logits are the input bit for bit (hook 5), and the input gradient is dz at the
    logits bit for bit (dz I), so every softmax form is read at the plan's surface."""
    N = _native()
    case = f"softmax-C{C_}-B{B}"
    z, y = R.softmax_rows(C_, B)
    v = np.random.default_rng(C_ + B).standard_normal((B, C_)).astype(np.float32)
    ref = R.softmax_ce(z, y, 1.0 / B)
    assert np.isfinite(ref["loss"]).all()
    ce_key = (FRAG4, 0, 0, 1, 0, EPI_SOFTMAX_CE)

    def run():
        out = {}
        with Mlp((C_, C_), (0,), (0,), (0,), B + 3) as plan:
            params, x, yb = _identity(plan, C_), Buf(z.shape, z), Buf(y.shape, y)
            st = N.stream_ptr()
            # lipasr_mlp_predict with probs, logits kept in the plan
            probs = Buf((B, C_))
            k2 = _snapshot()
            N.check(N.lib.lipasr_mlp_predict(plan.h, params.ptr(), None, x.ptr(), B, probs.ptr(), None, st))
            _assert_moved(k2, {SOFTMAX_CE: 1}, case + " predict")
            out["logits"], out["p_predict"] = plan.stage(0, 5, B), probs.read()
            onehot = Buf((B, C_))
            k2 = _snapshot()
            N.check(N.lib.lipasr_mlp_own_labels(plan.h, params.ptr(), None, x.ptr(), B, onehot.ptr(), st))
            _assert_moved(k2, {SOFTMAX_CE: 1}, case + " own_labels")
            torch.cuda.synchronize()
            out["onehot"] = onehot.read()
            # lipasr_mlp_output_vjp: on the logits and on the probabilities, with and without the probabilities out
            vb = Buf(v.shape, v)
            for on_logits in (0, 1):
                for with_p in (0, 1):
                    dx, pr = Buf((B, C_)), Buf((B, C_))
                    k2 = _snapshot()
                    N.check(N.lib.lipasr_mlp_output_vjp(plan.h, params.ptr(), None, x.ptr(), vb.ptr(), on_logits, B, pr.ptr() if with_p else None, dx.ptr(), st))
                    _assert_moved(k2, {SOFTMAX_VJP: 1}, case + " output_vjp")
                    torch.cuda.synchronize()
                    out[f"vjp{on_logits}{with_p}"] = dx.read()
                    out[f"vjp_dz{on_logits}{with_p}"] = plan.stage(0, 3, B)
                    if with_p:
                        out[f"vjp_p{on_logits}"] = pr.read()
            # lipasr_mlp_jacobian against lipasr_mlp_output_vjp with e_cls
            for on_logits in (0, 1):
                jac, pr = Buf((B, C_, C_)), Buf((B, C_))
                k2 = _snapshot()
                N.check(N.lib.lipasr_mlp_jacobian(plan.h, params.ptr(), None, x.ptr(), on_logits, B, pr.ptr(), jac.ptr(), C_ * C_, C_, st))
                _assert_moved(k2, {SOFTMAX_VJP_ONEHOT: C_}, case + " jacobian")
                torch.cuda.synchronize()
                out[f"jac{on_logits}"], out[f"jac_p{on_logits}"] = jac.read(), pr.read()
                rows = []
                for cls in range(C_):
                    e = np.zeros((B, C_), np.float32); e[:, cls] = 1.0
                    eb, dx = Buf(e.shape, e), Buf((B, C_))
                    N.check(N.lib.lipasr_mlp_output_vjp(plan.h, params.ptr(), None, x.ptr(), eb.ptr(), on_logits, B, None, dx.ptr(), st))
                    torch.cuda.synchronize()
                    rows.append(dx.read())
                    eb.read()
                out[f"jac_by_vjp{on_logits}"] = np.stack(rows, axis=1)
            # lipasr_mlp_train_fwd_bwd: EPI_BIAS_SOFTMAX_CE (loss rows, correct rows, the probabilities, dz at the logits)
            cfg = N.DropoutCfg()
            mdl = dict(x=z, y=y)
            for with_p in (1, 0):
                bufs = dict(params=params, bnstate=Buf((1,)), x=x, y=yb, grads=Buf((plan.n_params,)), loss=Buf((B,)), correct=Buf((B,)),
                            probs=Buf((B, C_)) if with_p else None)
                k2, gc = _snapshot(), _gemm(*ce_key)
                _train_call(plan, mdl, B, cfg, bufs=bufs)
                _assert_moved(k2, {}, case + " train_fwd_bwd")
                assert _gemm(*ce_key) == gc + 1
                out[f"train_dz{with_p}"], out[f"train_loss{with_p}"], out[f"train_correct{with_p}"] = plan.stage(0, 3, B), bufs["loss"].read(), bufs["correct"].read()
                out[f"train_p{with_p}"] = bufs["probs"].read() if with_p else plan.stage(0, 6, B)
                out[f"train_logits{with_p}"] = plan.stage(0, 5, B)
                bufs["grads"].read()
            # lipasr_mlp_input_grad: the counters say which softmax form ran -- the fused epilogue
            dx = Buf((B, C_))
            k2, gc = _snapshot(), _gemm(*ce_key)
            N.check(N.lib.lipasr_mlp_input_grad(plan.h, params.ptr(), None, x.ptr(), yb.ptr(), B, dx.ptr(), st))
            _assert_moved(k2, {}, case + " input_grad")
            assert _gemm(*ce_key) == gc + 1
            torch.cuda.synchronize()
            out["input_grad"] = dx.read()
            for b in (params, x, yb, vb):
                b.read()
        return out

    o = _twice(run)
    assert _same(o["logits"], z) and _same(o["train_logits1"], z) and _same(o["train_logits0"], z), "the logits are not the input"
    _held(case, (SOFTMAX_CE,), "p (predict)", o["p_predict"], ref["p"], ref["b_p"])
    assert np.array_equal(o["onehot"], ref["onehot"]), "own_labels: not the one-hot FIRST argmax"
    _record(case, (SOFTMAX_CE,), 0.0, "one-hot argmax")
    for on_logits in (0, 1):
        dz, bound, p, bp = R.softmax_vjp(z, v, on_logits)
        assert _same(o[f"vjp{on_logits}0"], o[f"vjp{on_logits}1"]), "the probabilities out change dz"
        assert _same(o[f"vjp_dz{on_logits}0"], o[f"vjp_dz{on_logits}1"])
        # dx = dz I: the same values; the matrix instruction adds a -0.0 onto +0.0 and may flush a subnormal, so zeros are
        # compared as values and what is below the smallest normal number may come out 0
        dxv, dzv = o[f"vjp{on_logits}1"], o[f"vjp_dz{on_logits}1"]
        tiny = np.abs(dzv) < R.TINY
        assert np.array_equal(dxv[~tiny], dzv[~tiny]) and (np.abs(dxv[tiny]) <= np.abs(dzv[tiny])).all(), "dx is not dz I"
        if on_logits:
            assert _same(dzv, v)
        else:
            _held(case, (SOFTMAX_VJP,), "p (v - p . v)", dzv, dz, bound)
            _held(case, (), "p (v - p . v) at the input", dxv, dz, bound)
        _held(case, (SOFTMAX_VJP,), "p (output_vjp)", o[f"vjp_p{on_logits}"], p, bp)
        assert _same(o[f"jac{on_logits}"], o[f"jac_by_vjp{on_logits}"]), "lipasr_mlp_jacobian is not softmax_vjp_kernel for e_cls, bit for bit"
        _held(case, (SOFTMAX_VJP_ONEHOT,), "p (jacobian)", o[f"jac_p{on_logits}"], p, bp)
        for cls in range(C_):
            e = np.zeros((B, C_), np.float32); e[:, cls] = 1.0
            dz, bound, _, _ = R.softmax_vjp(z, e, on_logits)
            if on_logits:
                assert _same(o["jac1"][:, cls], e)
            else:
                _held(case, (SOFTMAX_VJP_ONEHOT,), "p (e_cls - p_cls)", o["jac0"][:, cls], dz, bound)
    for with_p in (1, 0):
        what = "EPI_BIAS_SOFTMAX_CE "
        _held(case, (), what + "p", o[f"train_p{with_p}"], ref["p"], ref["b_p"])
        _held(case, (), what + "loss", o[f"train_loss{with_p}"], ref["loss"], ref["b_loss"])
        _held(case, (), what + "dz", o[f"train_dz{with_p}"], ref["dz"], ref["b_dz"])
        assert np.array_equal(o[f"train_correct{with_p}"], ref["correct"]), "correct rows: not [first argmax z == first argmax y]"
    assert _same(o["train_p1"], o["train_p0"]) and _same(o["train_dz1"], o["train_dz0"])
    _held(case, (), "EPI_BIAS_SOFTMAX_CE dz (input_grad)", o["input_grad"], ref["dz"], ref["b_dz"])
    if C_ > 1 and B > 4:
        assert abs(float(o["train_loss1"][4]) - 200.0) < 1e-3 and (o["train_p1"][4] == 0).sum() == C_ - 1  # p underflows, the loss does not


# ====================================================================================================== every kernel has a case
def test_every_k2_kernel_has_a_case(cuda):
    """The ids lipasr_debug_k2_launches knows against the claims above: a kernel added without a case fails here.  Prints (-s) per
    kernel the first case that showed it running and its worst error as a fraction of its bound.  It reads what the cases above
    recorded in this process (_ran, _worst), like the last test of the sibling instance suites: it belongs to a run of the whole
    file, and run alone or under a -k that leaves cases out it fails with "no case claims ...", as it should."""
    lib = _native().lib
    have = {k for k in range(64) if lib.lipasr_debug_k2_launches(k) >= 0}
    assert lib.lipasr_debug_k2_launches(-1) == -1 and lib.lipasr_debug_k2_launches(len(K2_NAMES)) == -1
    assert have == set(range(len(K2_NAMES))), "the library knows K2 ids this file has no name for"
    unclaimed = sorted(have - set(_ran))
    assert not unclaimed, "no case claims " + ", ".join(K2_NAMES[k] for k in unclaimed)
    for k in sorted(have):
        assert lib.lipasr_debug_k2_launches(k) > 0
        fr, where, what = _worst.get(k, (float("nan"), "-", "-"))
        print(f"{K2_NAMES[k]}: {lib.lipasr_debug_k2_launches(k)} launches, first shown by {_ran[k]}; worst {fr:.3f} of its bound ({what}, {where})")
    for what, why in UNREACHABLE.items():
        print(f"unreachable: {what}: {why}")
