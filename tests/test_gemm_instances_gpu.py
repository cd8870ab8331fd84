"""Every GEMM kernel instance against float64, and proof of which instance ran.

The gemm_*.hip tile units instantiate about sixty kernels (GemmTable: [kind][exchange epilogue][AMODE][BMODE][arithmetic], plus the grouped
weight-gradient kernels) and pick_gemm / launch_gemm_group_tn choose between them from the shape, the alignment, the arithmetic
mode, the plan's tile threshold and CU budget, an occupancy query and the lipasr_debug_gemm_mode bits.  The cases below are kept
in two module-level tables; every case names the instances (and epilogues) it is meant to run, the launch counters
(lipasr_debug_gemm_launches / lipasr_debug_group_launches) must say that those ran, and a last test checks that the tables
cover every instance the library reports.

  * PLAIN_CASES: single launches through lipasr_debug_gemm against the float64 product (numpy).
  * PLAN_CASES:  one training step through the plan against oracle.mlp_ref.forward_backward in float64, with injected dropout
                 masks; arithmetic mode 1 against the same oracle with the GEMM operands rounded to bf16.
  * the inference epilogues at ragged shapes against the oracle's inference functions.

Every case sets every knob itself, so LIPASR_GEMM_MODE / LIPASR_FUSE_BN / LIPASR_GEMM_TILES / LIPASR_COMPUTE in the environment do
not change what it covers.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import build_model, dev, grads_of, load_params, read_params, rel_err
from oracle import attacks_ref as A
from oracle import mlp_ref as P

gpu = pytest.mark.gpu

# GemmKind and Epi of csrc/gemm.h (documented at lipasr_debug_gemm_launches in include/lipasr.h)
FRAG4, FRAG16, LDS, RING, RING_X1, RING2 = range(6)
KINDS = ("FRAG4", "FRAG16", "LDS", "RING", "RING_X1", "RING2")
(EPI_STORE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RELU_BN, EPI_DZ_INFER, EPI_SIGNSTEP, EPI_BIAS_RELU_STATS, EPI_DH_STATS, EPI_DZ_NOBN,
 EPI_BIAS_SOFTMAX_CE, EPI_BIAS_RELU_BNX, EPI_DH_BNX) = range(12)
N_EPI = 12
# grouped weight-gradient launches: ("group", family, arithmetic, variant) -- family 0 fragment tiles, 1 LDS tiles, 2 the ring kernel
# (variant -1 launches; 1 / 2 / 3 problems on 64x64 ring, 128x128 split-pass, 128x128 per-fragment tiles; 0 riders on plain tiles)
GROUP_KEYS = ([("group", f, a, -1) for f in (0, 1) for a in (0, 1, 2)] + [("group", 2, 2, v) for v in (-1, 0, 1, 2, 3)])

_open_models = []


def _native():
    from lipasr import _native as N

    return N


@pytest.fixture(autouse=True)
def _default_knobs_and_closed_models():
    yield
    _native().lib.lipasr_debug_gemm_mode(0)
    while _open_models:
        _open_models.pop().close()


def g(kind, exchange, amode, bmode, arith, epi):
    return (kind, exchange, amode, bmode, arith, epi)


def grp(family, arith, variant=-1):
    return ("group", family, arith, variant)


def _key_name(k):
    if k[0] == "group":
        return f"grouped {('fragment', 'LDS', 'ring')[k[1]]} arith {k[2]} variant {k[3]}"
    return f"{KINDS[k[0]]}{' exchange' if k[1] else ''} AMODE {k[2]} BMODE {k[3]} arith {k[4]}" + (f" epilogue {k[5]}" if len(k) > 5 else "")


@functools.lru_cache(maxsize=None)
def _instances():
    """Every (kind, exchange, AMODE, BMODE, arithmetic) the library has a kernel for."""
    lib = _native().lib
    return tuple((k, x, a, b, ar) for k in range(6) for x in (0, 1) for a in (0, 1) for b in (0, 1) for ar in (0, 1, 2)
                 if lib.lipasr_debug_gemm_launches(k, x, a, b, ar, -1) >= 0)


def _snapshot():
    lib = _native().lib
    s = {inst + (e,): lib.lipasr_debug_gemm_launches(*inst, e) for inst in _instances() for e in range(N_EPI)}
    s.update({k: lib.lipasr_debug_group_launches(*k[1:]) for k in GROUP_KEYS})
    return s


def _moved(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


# =================================================================================================
# 1. single launches against the float64 product
# =================================================================================================
SENTINEL = -12345.0


def _layout(amode, bmode):
    return (amode, 0 if bmode else 1)  # (transA, transB) of the C entry: amode = transA, bmode = !transB


# (id, kind, arithmetic, knob bits 0-1, (M, N, K), (pad of lda, pad of ldb), why this shape)
_PLAIN_SHAPES = [
    ("frag4", FRAG4, (0, 1, 2), 1, (70, 45, 37), (0, 0), "3 x 2 tiles of 32, ragged in M (6 rows) and N (13 columns); K = 4 x 8 + 5"),
    ("frag16", FRAG16, (0, 1, 2), 1, (70, 45, 531), (0, 0), "the deep rule (<= 192 tiles, K >= 512): 16 wavefronts split K; tail 531 = 66 x 8 + 3"),
    ("lds", LDS, (0, 1, 2), 2, (150, 70, 75), (0, 0), "3 x 2 tiles of 64, ragged (22 rows, 6 columns); K = 2 x 32 + 11, and no multiple of 4: not ring-legal in mode 2"),
    ("ring", RING, (2,), 2, (152, 72, 192), (0, 0), "6 k-steps of 32 > 4 ring stages: the ring wraps; M, N, leading dimensions multiples of 4"),
    ("ring-ktail", RING, (2,), 2, (152, 72, 196), (0, 0), "the same with a 4-wide K tail that reads the zeros source"),
    ("ring-illegal-lda", LDS, (2,), 2, (152, 72, 192), (1, 0), "an odd leading dimension of A is not ring-legal: falls to the LDS tile"),
    ("ring-illegal-ldb", LDS, (2,), 2, (152, 72, 192), (0, 3), "a leading dimension of B that is no multiple of 4: falls to the LDS tile"),
]
PLAIN_CASES = [dict(id=f"{name}-a{ar}-A{am}B{bm}", kind=kind, arith=ar, knob=knob, shape=shape, pads=pads, amode=am, bmode=bm,
                    claims=[g(kind, 0, am, bm, ar, EPI_STORE)], why=why)
               for name, kind, ariths, knob, shape, pads, why in _PLAIN_SHAPES for ar in ariths for am in (0, 1) for bm in (0, 1)]


def _stored(x, pad):
    """x on the device in rows of x.shape[1] + pad floats; the padding is NaN (a kernel that reads it poisons its result)."""
    t = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device="cuda")
    t[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t


def _debug_gemm(case, a, b, scale=1.0, c_pad=5):
    """op(A) = a [M, K], op(B) = b [K, N] through lipasr_debug_gemm in the case's layout; C has ldc = N + c_pad and two rows more than
    M, prefilled with a sentinel that must survive.  Asserts that exactly the case's instance took exactly one launch."""
    N = _native()
    h = N.get_handle(0)
    ta, tb = _layout(case["amode"], case["bmode"])
    At = _stored(a.T if ta else a, case["pads"][0])
    Bt = _stored(b.T if tb else b, case["pads"][1])
    M, K_ = a.shape
    Nn = b.shape[1]
    ldc = Nn + c_pad
    out = torch.full((M + 2, ldc), SENTINEL, device="cuda")
    N.check(N.lib.lipasr_debug_gemm_mode(case["knob"]))
    before = _snapshot()
    N.check(N.lib.lipasr_debug_gemm(h.h, case["arith"], ta, tb, M, Nn, K_, N.ptr(At), At.shape[1], N.ptr(Bt), Bt.shape[1], N.ptr(out), ldc,
                                    scale, scale, N.stream_ptr()))
    o = out.cpu().numpy()
    moved = _moved(before, _snapshot())
    assert moved == {k: 1 for k in case["claims"]}, {_key_name(k): v for k, v in moved.items()}
    assert (o[:M, Nn:] == SENTINEL).all(), "the padding of C's rows was written"
    assert (o[M:] == SENTINEL).all(), "rows after M were written"
    return o[:M, :Nn].astype(np.float64)


def _abs_product(a, b):
    return np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)


@gpu
@pytest.mark.parametrize("case", PLAIN_CASES, ids=[c["id"] for c in PLAIN_CASES])
def test_single_launch_against_float64(cuda, case):
    """One launch per check through lipasr_debug_gemm.  Small integers are exact in every arithmetic (they are bf16 and fp16
    numbers): a wrong lane, swizzle or C map fails outright.  Random operands per element against float64: mode 0 within
    4e-7 sum |a||b|, mode 2 within 6e-7 (the project's bounds); mode 1 against the float64 product of the operands rounded to bf16
    (ties to even) within the mode-0 bound, since products of bf16 numbers are exact in fp32 -- once with bf16-exact operands
    (the contraction) and once with general ones (the rounding is to nearest even, not truncation); mode 2 also at the two ends
    of the operand range the header documents (N(0,1) 2^-3 and N(0,1) 2^12 at scale 1)."""
    M, N_, K_ = case["shape"]
    ar = case["arith"]
    rng = np.random.default_rng(M + 7 * N_ + 13 * K_ + 101 * ar)
    ai = rng.integers(-3, 4, (M, K_)).astype(np.float32)
    bi = rng.integers(-3, 4, (K_, N_)).astype(np.float32)
    # (ldc = N + 8: rows of C stay 16-byte aligned where N allows it, so the vector store path runs here and the scalar one below)
    np.testing.assert_array_equal(_debug_gemm(case, ai, bi, scale=16.0 if ar == 2 else 1.0, c_pad=8), ai.astype(np.float64) @ bi.astype(np.float64))
    a = rng.standard_normal((M, K_)).astype(np.float32)
    b = rng.standard_normal((K_, N_)).astype(np.float32)

    def check(a, b, rel, scale=1.0, what=""):
        got = _debug_gemm(case, a, b, scale=scale)
        ra, rb = (P.round_bf16(a), P.round_bf16(b)) if ar == 1 else (a, b)
        ref = ra.astype(np.float64) @ rb.astype(np.float64)
        bound = rel * _abs_product(ra, rb) + 1e-30
        worst = float((np.abs(got - ref) / bound).max())
        assert worst <= 1.0, f"{what}: {worst:.3g} of the bound, at {np.unravel_index(np.argmax(np.abs(got - ref) / bound), ref.shape)}"

    if ar == 0:
        check(a, b, 4e-7, what="fp32")
    elif ar == 1:
        check(P.round_bf16(a), P.round_bf16(b), 4e-7, what="bf16-exact operands")
        check(a, b, 4e-7, what="general operands (round to nearest even)")
    else:
        check(a, b, 6e-7, scale=16.0, what="fp16 split, scale 16")
        check(a * np.float32(2.0 ** -3), b * np.float32(2.0 ** -3), 6e-7, what="fp16 split, operands 2^-3, scale 1")
        check(a * np.float32(2.0 ** 12), b * np.float32(2.0 ** 12), 6e-7, what="fp16 split, operands 2^12, scale 1")


@gpu
def test_debug_gemm_rejects_bad_arguments(cuda):
    N = _native()
    h = N.get_handle(0)
    t = torch.zeros(4, 4, device="cuda")
    args = (N.ptr(t), 4, N.ptr(t), 4, N.ptr(t), 4)
    assert N.lib.lipasr_debug_gemm(h.h, 3, 0, 0, 4, 4, 4, *args, 1.0, 1.0, N.stream_ptr()) == N.EINVAL
    assert N.lib.lipasr_debug_gemm(h.h, -1, 0, 0, 4, 4, 4, *args, 1.0, 1.0, N.stream_ptr()) == N.EINVAL
    assert N.lib.lipasr_debug_gemm(h.h, 2, 0, 0, 4, 4, 4, *args, 3.0, 1.0, N.stream_ptr()) == N.EINVAL  # mode 2: powers of two only
    assert N.lib.lipasr_debug_gemm(h.h, 1, 0, 0, 4, 4, 4, *args, 3.0, 0.0, N.stream_ptr()) == N.OK       # other modes do not read them
    assert N.lib.lipasr_debug_gemm_launches(FRAG16, 1, 0, 0, 0, -1) == -1   # no such instance
    assert N.lib.lipasr_debug_gemm_launches(FRAG4, 0, 0, 0, 0, N_EPI) == -1
    assert N.lib.lipasr_debug_group_launches(2, 0, -1) == -1 and N.lib.lipasr_debug_group_launches(3, 0, -1) == -1


# =================================================================================================
# 2. one training step through the plan against the float64 oracle
# =================================================================================================
def _state(spec, seed, nonneg=True):
    """Parameters with every field away from its default (biases, gamma, beta, moving statistics)."""
    p = P.init_params(spec, seed=seed, dtype=np.float32, nonneg_init=nonneg)
    rng = np.random.default_rng(seed + 100)
    for l, s in enumerate(spec):
        p.b[l] = (0.1 * rng.standard_normal(s.n_out)).astype(np.float32)
        if s.bn:
            p.gamma[l] = (1 + 0.2 * rng.standard_normal(s.n_out)).astype(np.float32)
            p.beta[l] = (0.1 * rng.standard_normal(s.n_out)).astype(np.float32)
            p.mov_mean[l] = (0.5 + 0.1 * rng.standard_normal(s.n_out)).astype(np.float32)
            p.mov_var[l] = rng.uniform(0.5, 1.5, s.n_out).astype(np.float32)
    return p


def _spec(widths, bn_off, drop):
    n = len(widths) - 1
    return [P.LayerSpec(widths[i], widths[i + 1], i < n - 1 and i not in bn_off, 0.1 if i in drop else 0.0, True) for i in range(n)]


@functools.lru_cache(maxsize=None)
def _problem(widths, bn_off, drop, batch, seed=4):
    """Model, batch and dropout masks of a case (shared by every case on the same shape and seed; read-only)."""
    spec = _spec(widths, bn_off, drop)
    p = _state(spec, seed)
    rng = np.random.default_rng(batch + len(widths) + 1000 * (seed - 4))
    x = rng.standard_normal((batch, widths[0])).astype(np.float32)
    y = P.to_categorical(rng.integers(0, widths[-1], batch), widths[-1])
    masks = [((rng.uniform(size=(batch, s.n_out)) > s.dropout) / (1 - s.dropout)).astype(np.float32) if s.dropout > 0 else None for s in spec]
    return spec, p, x, y, masks


def _loss_rows(ref, y):
    z = ref["logits"] - ref["logits"].max(axis=1, keepdims=True)
    return -(y * (z - np.log(np.exp(z).sum(axis=1, keepdims=True)))).sum(axis=1)


def _tensors(spec, p, ref, y):
    """What a training step leaves, as {name: array}: gradients, loss rows, moving statistics after the forward pass."""
    t = {"loss_rows": _loss_rows(ref, y)}
    for l, s in enumerate(spec):
        t[f"dW{l}"], t[f"db{l}"] = ref["dW"][l], ref["db"][l]
        if s.bn:
            mu, var = ref["stats"][l]
            t[f"dgamma{l}"], t[f"dbeta{l}"] = ref["dgamma"][l], ref["dbeta"][l]
            t[f"mov_mean{l}"] = p.mov_mean[l] * P.BN_MOMENTUM + mu * (1 - P.BN_MOMENTUM)
            t[f"mov_var{l}"] = p.mov_var[l] * P.BN_MOMENTUM + var * (1 - P.BN_MOMENTUM)
    return t


@functools.lru_cache(maxsize=None)
def _reference(widths, bn_off, drop, batch, bf16, seed=4):
    """The oracle in float64 (bf16: with the operands of every matrix product rounded to bf16) -> (tensors, correct rows, d_ref).
    d_ref (bf16 only): per tensor, the rel_err between that oracle in float64 and with every intermediate held in float32 -- how far
    rounding flips alone move the result."""
    spec, p, x, y, masks = _problem(widths, bn_off, drop, batch, seed)
    rnd = P.round_bf16 if bf16 else None
    p64 = p.astype(np.float64)
    ref = P.forward_backward(spec, p64, x.astype(np.float64), y.astype(np.float64), masks=masks, training=True, round_operands=rnd)
    t64 = _tensors(spec, p64, ref, y.astype(np.float64))
    correct = (ref["prob"].argmax(1) == y.argmax(1)).astype(np.float32)
    d_ref = None
    if bf16:
        r32 = P.forward_backward(spec, p, x, y, masks=masks, training=True, round_operands=rnd)
        t32 = _tensors(spec, p, r32, y)
        assert all(v.dtype == np.float32 for v in t32.values())
        d_ref = {k: _err(k, t32[k], t64[k]) for k in t64}
    return t64, correct, d_ref


# The bf16 problems are chosen decisive where that can be had.  A computed operand (an activation, a gradient) that lies within
# fp32 resolution of the middle between two bf16 numbers rounds either way in a correct fp32 implementation, and with 150 signed
# terms to a weight-gradient element one such flip (2^-8 of the operand) moves that element by several 1e-4 of the tensor's
# maximum: more than d_ref, which sees only the flips of numpy's own float32 evaluation.  (Seed 4 of W_LDS has such an operand:
# an activation of layer 1 lies 4.3e-8 of its value from the middle, under the 6e-8 that fp32 resolves; the LDS kernels round it
# the other way and dW2 moves by 4.5e-4.)  So the seed of a bf16 problem is taken, from the oracle alone, as one whose result does
# not hang on such flips: with every computed operand (not the inputs and kernels, which both sides hold exactly) moved before its
# rounding by a relative FLIP_ETA, uniformly drawn, FLIP_TRIALS times, no tensor moves by its fp32 bound.  FLIP_ETA = 2^-22 is four
# units of fp32 rounding: the unit for a value that fp32 holds, times the 4 that the bounds allow a summation order other than
# numpy's.  The seed is also one at which numpy's float32 evaluation flips nothing that matters (4 d_ref under the fp32 bound of
# every tensor), so these cases are held to the fp32 bounds themselves.  Both narrow what can flip and cannot exclude it: an
# operand computed with a larger error can still flip, and then the case fails at its bound and names the element.
# test_bf16_problems_are_decisive holds the seeds to both without a GPU.
# W_WIDE (2 10^5 computed operands, against 2 10^4 and 8 10^4) stays on seed 4: of 1500 seeds none met the criterion.
FLIP_ETA = 2.0 ** -22
FLIP_TRIALS = 24


def _flip_sensitivity(widths, bn_off, drop, batch, seed, eta=FLIP_ETA, trials=FLIP_TRIALS):
    """Largest move of a tensor of the bf16 oracle, as a share of its fp32 bound, under `trials` draws of relative noise `eta` on
    every computed GEMM operand before it is rounded to bf16."""
    spec, p, x, y, masks = _problem(widths, bn_off, drop, batch, seed)
    p64, x64, y64 = p.astype(np.float64), x.astype(np.float64), y.astype(np.float64)
    given = {id(x64)} | {id(w) for w in p64.W}
    t64 = _tensors(spec, p64, P.forward_backward(spec, p64, x64, y64, masks=masks, training=True, round_operands=P.round_bf16), y64)
    worst = 0.0
    for trial in range(trials):
        rng = np.random.default_rng(trial)

        def rnd(a):
            return P.round_bf16(a if id(a) in given else a * (1 + eta * rng.uniform(-1, 1, a.shape)))

        t = _tensors(spec, p64, P.forward_backward(spec, p64, x64, y64, masks=masks, training=True, round_operands=rnd), y64)
        worst = max(worst, max(_err(k, t[k], t64[k]) / _fp32_bound(k) for k in t64))
    return worst


def _err(name, got, ref):
    if name == "loss_rows":  # relative to max(1, |loss|)
        return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(1.0, np.abs(ref).max()))
    return rel_err(got, ref)


def _fp32_bound(name):
    """The project's bounds against the float64 oracle (test_mlp_gpu.py): dW, db 5e-5 of the tensor's maximum; dgamma, dbeta 3e-4 (sums
    of `batch` signed terms that cancel); loss 1e-4 max(1, |loss|); moving statistics 1e-5 (test_small_case_against_golden)."""
    if name.startswith(("dgamma", "dbeta")):
        return 3e-4
    if name.startswith("loss"):
        return 1e-4
    return 1e-5 if name.startswith("mov_") else 5e-5


def _plan_case(id, widths, batch, arith, fuse, tiles, cus, knob, claims, why, bn_off=(), drop=(0, 1), form="step"):
    seed = BF16_SEEDS[tuple(widths)] if arith == 1 else 4
    return dict(id=id, widths=tuple(widths), batch=batch, arith=arith, fuse=fuse, tiles=tiles, cus=cus, knob=knob, claims=list(claims), why=why,
                bn_off=tuple(bn_off), drop=tuple(drop), form=form, seed=seed)


W_SMALL = (100, 72, 50, 33, 10)        # widths that are no multiple of 32 (72, 50, 33) or of 4 (50, 33): fragment tiles only at batch 77
W_LDS = (100, 136, 72, 70, 10)         # 136 = 2 x 64 + 8 and 72 = 64 + 8 columns; K = 100 / 136 / 72 / 70: tails of the 32-wide k-step;
                                       # 70 is no multiple of 4, which keeps layer 2 and the gradient into layer 1 off the ring in mode 2
W_WIDE = (512, 1000, 10)               # weight gradient 513 x 1000 (the ones row alone in a last tile, a last column block of 40), K = batch
BF16_SEEDS = {W_SMALL: 6, W_LDS: 30, W_WIDE: 4}   # seeds of the bf16 problems: decisive ones (see FLIP_ETA) but for W_WIDE
KNOB_SPLIT_DW0, KNOB_NO_RING, KNOB_RING64, KNOB_RING128F, KNOB_NO_X1 = 4, 32, 64, 128, 512


def _small_claims(a, fuse):
    """W_SMALL at batch 77: 3 row tiles of 32 (13 rows in the last), 3 / 2 / 2 column tiles (8 / 18 / 1 columns in the last)."""
    c = [g(FRAG4, fuse, 0, 1, a, EPI_BIAS_RELU_BNX if fuse else EPI_BIAS_RELU_STATS), g(FRAG4, 0, 0, 1, a, EPI_BIAS_SOFTMAX_CE),
         g(FRAG4, fuse, 0, 0, a, EPI_DH_BNX if fuse else EPI_DH_STATS), grp(0, a)]
    if a < 2:  # layer 2 without BatchNorm (mode 2 needs it everywhere)
        c += [g(FRAG4, 0, 0, 1, a, EPI_BIAS_RELU), g(FRAG4, 0, 0, 0, a, EPI_DZ_NOBN)]
    return c


def _lds_claims(a, fuse, big=LDS):
    """W_LDS at batch 150 (3 row tiles of 64, 22 rows in the last) with lipasr_mlp_set_gemm_tiles(1).  `big`: the instance of the
    ring-legal layers in mode 2.  The gradient into layer 2 has K = 10 < 32: fragment tiles."""
    fw, bw = (EPI_BIAS_RELU_BNX, EPI_DH_BNX) if fuse else (EPI_BIAS_RELU_STATS, EPI_DH_STATS)
    c = [g(FRAG4, 0, 0, 1, a, EPI_BIAS_SOFTMAX_CE), g(FRAG4, fuse, 0, 0, a, bw), grp(0, a)]
    if a < 2:  # layer 1 without BatchNorm
        c += [g(LDS, fuse, 0, 1, a, fw), g(LDS, fuse, 0, 0, a, bw), g(LDS, 0, 0, 1, a, EPI_BIAS_RELU), g(LDS, 0, 0, 0, a, EPI_DZ_NOBN)]
    else:      # layers 0, 1 and the gradient into layer 0 are ring-legal; layer 2 (70 columns) and the gradient into layer 1 (lda 70) are not
        c += [g(big, fuse, 0, 1, 2, fw), g(big, fuse, 0, 0, 2, bw), g(LDS, fuse, 0, 1, 2, fw), g(LDS, fuse, 0, 0, 2, bw)]
    return c


def _wide_claims(a, fwd=FRAG4):
    """W_WIDE at batch 100: forward 100 x 1000 x 512 (32 tiles of 64: below the default threshold of 224), gradient into layer 0 with K = 10."""
    return [g(fwd, 0, 0, 1, a, EPI_BIAS_RELU_STATS), g(FRAG4, 0, 0, 1, a, EPI_BIAS_SOFTMAX_CE), g(FRAG4, 0, 0, 0, a, EPI_DH_STATS)]


PLAN_CASES = (
    [_plan_case(f"chain-frag-a{a}", W_SMALL, 77, a, 0, 0, 0, 0, _small_claims(a, 0), "launch chain on fragment tiles: the STATS epilogues' column sums per 32-row tile",
                bn_off=(2,) if a < 2 else (), drop=(0, 1, 2)) for a in (0, 1, 2)]
    + [_plan_case(f"chain-lds-a{a}", W_LDS, 150, a, 0, 1, 0, 0, _lds_claims(a, 0, RING), "launch chain on 64 x 64 tiles (mode 2: the ring for the legal layers)",
                  bn_off=(1,) if a < 2 else (), drop=(0, 1, 2)) for a in (0, 1, 2)]
    + [_plan_case(f"exchange-frag-a{a}", W_SMALL, 77, a, 1, 0, 0, 0, _small_claims(a, 1), "exchange epilogue on fragment tiles",
                  bn_off=(2,) if a < 2 else (), drop=(0, 1, 2)) for a in (0, 1, 2)]
    + [_plan_case(f"exchange-lds-a{a}", W_LDS, 150, a, 1, 1, 0, 0, _lds_claims(a, 1), "exchange epilogue on LDS tiles", bn_off=(1,), drop=(0, 1, 2)) for a in (0, 1)]
    + [_plan_case("exchange-ring-x1", W_LDS, 150, 2, 1, 1, 0, 0, _lds_claims(2, 1, RING_X1),
                  "whole device, 9 and 6 tiles <= CUs: the loader-wavefront instance; layer 2 keeps the LDS exchange tile in mode 2", drop=(0, 1, 2)),
       _plan_case("exchange-ring", W_LDS, 150, 2, 1, 1, 0, KNOB_NO_X1, _lds_claims(2, 1, RING), "the same without the loader-wavefront instance (bit 9): the 64 x 64 ring exchange tile",
                  drop=(0, 1, 2)),
       # batch 300 = two 128-row tiles + 44 rows; layer 0 (136 columns) and the gradient into it make 3 x 3 = 9 tiles of 128 x 64 on a budget of
       # 10 CUs (3 cus <= 4 tiles, tiles <= cus); layer 1 (72 columns: 6 such tiles, too few) takes RING_X1 with its 10 tiles of 64 x 64
       _plan_case("exchange-ring2", W_LDS, 300, 2, 1, 1, 10, 0, _lds_claims(2, 1, RING2) + [g(RING_X1, 1, 0, 1, 2, EPI_BIAS_RELU_BNX)],
                  "128 x 64 exchange tiles on a CU share, ragged last row tile", drop=(0, 1, 2))]
    # grouped weight gradients on 64 x 64 tiles: 144 + 16 tiles >= 128, K = 100 = 3 x 32 + 4
    + [_plan_case(f"group-lds-a{a}", W_WIDE, 100, a, 0, 0, 0, 0, _wide_claims(a) + [grp(1, a)], "grouped weight gradients on LDS tiles", drop=(0,)) for a in (0, 1)]
    + [_plan_case("group-lds-a2", W_WIDE, 100, 2, 0, 0, 0, KNOB_NO_RING, _wide_claims(2) + [grp(1, 2)], "mode 2 without the ring (bit 5): the grouped LDS kernel's third arithmetic", drop=(0,)),
       _plan_case("group-ring-64", W_WIDE, 100, 2, 0, 0, 0, KNOB_RING64, _wide_claims(2) + [grp(2, 2), grp(2, 2, 1), grp(2, 2, 0)],
                  "64 x 64 ring tiles (bit 6); the 10-class layer is not ring-legal and rides on plain tiles", drop=(0,)),
       _plan_case("group-ring-128-split-pass", W_WIDE, 100, 2, 0, 0, 64, 0, _wide_claims(2) + [grp(2, 2), grp(2, 2, 2), grp(2, 2, 0)],
                  "40 tiles of 128 x 128 cover 40 % of a 64-CU budget: the split-pass tile", drop=(0,)),
       _plan_case("group-ring-128-per-fragment", W_WIDE, 100, 2, 0, 0, 64, KNOB_RING128F, _wide_claims(2) + [grp(2, 2), grp(2, 2, 3), grp(2, 2, 0)],
                  "the 128 x 128 tile that splits per fragment (bit 7)", drop=(0,))]
    # the first layer's [dW; db] as a launch of its own (AMODE 1, BMODE 1, ones_row): 513 = 16 x 32 + 1 rows, the ones row alone in a tile
    + [_plan_case(f"split-dw0-frag-a{a}", W_WIDE, 100, a, 0, 0, 0, KNOB_SPLIT_DW0, _wide_claims(a) + [grp(0, a), g(FRAG4, 0, 1, 1, a, EPI_STORE)],
                  "knob bit 2: layer 0's weight gradient through launch_gemm on fragment tiles (144 tiles of 64 < 224)", drop=(0,)) for a in (0, 1, 2)]
    + [_plan_case(f"head-dw0-lds-a{a}", W_WIDE, 100, a, 0, 0, 0, 2, _wide_claims(a, RING if a == 2 else LDS) + [grp(0, a), g(RING if a == 2 else LDS, 0, 1, 1, a, EPI_STORE)],
                  "train_fwd_bwd_head + train_dw0 with the LDS kernel forced (knob bits 0-1 = 2): 64 x 64 tiles (mode 2: the ring) with ones_row", drop=(0,), form="head+dw0")
       for a in (0, 1, 2)]
)


def _model(spec, max_batch, arith, fuse, tiles, cus, knob):
    N = _native()
    assert cus <= torch.cuda.get_device_properties(0).multi_processor_count, "a CU budget above the device would break the exchange's residency"
    m = build_model(spec, max_batch=max_batch, compute_dtype="float32")
    _open_models.append(m)
    N.check(N.lib.lipasr_mlp_set_compute(m._plan, arith))
    N.check(N.lib.lipasr_mlp_set_fuse_bn(m._plan, fuse))
    N.check(N.lib.lipasr_mlp_set_gemm_tiles(m._plan, tiles))
    N.check(N.lib.lipasr_mlp_set_cu_budget(m._plan, cus))
    N.check(N.lib.lipasr_debug_gemm_mode(knob))
    return m


def open_plan_case(case):
    """The case's model with its parameters loaded and every knob set -> (model, spec, x, y, masks), the last three on the device."""
    spec, p, x, y, masks = _problem(case["widths"], case["bn_off"], case["drop"], case["batch"], case["seed"])
    m = _model(spec, case["batch"], case["arith"], case["fuse"], case["tiles"], case["cus"], case["knob"])
    load_params(m, p)
    return m, spec, dev(x), dev(y), [dev(k) if k is not None else None for k in masks]


def run_plan_case(case):
    """One training step of the case; returns (tensors the step left, correct rows, the launch counters that moved)."""
    m, spec, xt, yt, mt = open_plan_case(case)
    before = _snapshot()
    if case["form"] == "head+dw0":
        m.train_fwd_bwd(xt, yt, masks=mt, defer_dw0=True)
        m.train_dw0(xt)
    else:
        m.train_fwd_bwd(xt, yt, masks=mt)
    errors = m.exchange_errors()  # (synchronises)
    moved = _moved(before, _snapshot())
    assert errors == 0, "an exchange gave up"
    return step_tensors(m, spec, case["batch"]) + (moved,)


def step_tensors(m, spec, batch):
    """What the model's last training step left -> (tensors by the names of _tensors, correct rows)."""
    got = grads_of(m, spec)
    after = read_params(m, spec)
    t = {"loss_rows": m._loss_rows[:batch].cpu().numpy().astype(np.float64)}
    for l, s in enumerate(spec):
        t[f"dW{l}"], t[f"db{l}"] = got["dW"][l], got["db"][l]
        if s.bn:
            t[f"dgamma{l}"], t[f"dbeta{l}"] = got["dgamma"][l], got["dbeta"][l]
            t[f"mov_mean{l}"], t[f"mov_var{l}"] = after.mov_mean[l], after.mov_var[l]
    return t, m._correct_rows[:batch].cpu().numpy()


@gpu
@pytest.mark.parametrize("case", PLAN_CASES, ids=[c["id"] for c in PLAN_CASES])
def test_training_step_against_float64_oracle(cuda, case):
    """One train_fwd_bwd with injected dropout masks against oracle.mlp_ref.forward_backward in float64: every gradient, the loss
    rows, the correct rows and the moving statistics, on the (instance, epilogue) pairs the case claims (their counters must have moved).

    Modes 0 and 2 are held to the project's fp32 bounds (_fp32_bound).  Mode 1 is compared with the oracle whose GEMM operands are
    rounded to bf16; a rounding flip moves an element by 2^-9, so its bound comes from the reference alone: d_ref, the distance
    between that oracle in float64 and in float32, per tensor; the bound is max(4 d_ref, the fp32 bound) -- 4 for a summation order
    other than numpy's.  d_ref and the observed errors are printed.  The bf16 problems are decisive ones where that can be had (FLIP_ETA)."""
    bf16 = case["arith"] == 1
    want, correct, d_ref = _reference(case["widths"], case["bn_off"], case["drop"], case["batch"], bf16, case["seed"])
    got, got_correct, moved = run_plan_case(case)
    missing = set(case["claims"]) - set(moved)
    print(f"{case['id']} ran: " + ", ".join(_key_name(k) for k in sorted(moved, key=str)))
    assert not missing, "claimed but did not run: " + ", ".join(_key_name(k) for k in sorted(missing, key=str))
    failed = []
    for name in want:
        err = _err(name, got[name], want[name])
        bound = max(4 * d_ref[name], _fp32_bound(name)) if bf16 else _fp32_bound(name)
        if bf16:
            print(f"{case['id']} {name}: d_ref {d_ref[name]:.3e} observed {err:.3e} bound {bound:.3e}")
        if not err < bound:
            where = np.unravel_index(np.argmax(np.abs(got[name] - want[name])), want[name].shape)
            failed.append(f"{name}: {err:.3e} >= {bound:.3e} at {where}")
    assert not failed, failed
    np.testing.assert_array_equal(got_correct, correct)


def test_bf16_problems_are_decisive():
    """(no GPU) No tensor of a bf16 problem's oracle moves by its fp32 bound when every computed operand is moved by fp32-sized
    noise before it is rounded to bf16: what the bf16 cases compare does not hang on a rounding that fp32 cannot decide."""
    problems = {(c["widths"], c["bn_off"], c["drop"], c["batch"], c["seed"]) for c in PLAN_CASES if c["arith"] == 1 and c["widths"] != W_WIDE}
    assert len(problems) == 2
    for prob in sorted(problems):
        worst = _flip_sensitivity(*prob)
        d_ref = _reference(*prob[:4], True, prob[4])[2]
        flips32 = max(4 * d_ref[k] / _fp32_bound(k) for k in d_ref)
        print(f"widths {prob[0]} batch {prob[3]} seed {prob[4]}: noise moves {worst:.3g}, 4 d_ref is {flips32:.3g} of the fp32 bound")
        assert worst < 1.0 and flips32 < 1.0, prob


# =================================================================================================
# 3. the inference epilogues at ragged shapes
# =================================================================================================
INFER_CASES = [
    dict(id="infer-frag", knob=1, why="fragment tiles: 3 x 3 / 2 / 2 / 1 tiles of 32 at batch 77",
         claims={"predict": [g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS)],
                 "input_grad": [g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_SOFTMAX_CE), g(FRAG4, 0, 0, 0, 0, EPI_DZ_INFER), g(FRAG4, 0, 0, 0, 0, EPI_STORE)],
                 "attack_step": [g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_SOFTMAX_CE), g(FRAG4, 0, 0, 0, 0, EPI_DZ_INFER), g(FRAG4, 0, 0, 0, 0, EPI_SIGNSTEP)],
                 "output_vjp": [g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS), g(FRAG4, 0, 0, 0, 0, EPI_DZ_INFER), g(FRAG4, 0, 0, 0, 0, EPI_STORE)]}),
    # knob 2: layer 0 (77 x 72 x 100) and the gradients into layers 0 and -- as the last GEMM -- the input (77 x 72 x 50, 77 x 100 x 72) are
    # LDS-legal (M, N >= 64, K >= 32); the narrower ones stay on fragment tiles
    dict(id="infer-lds", knob=2, why="LDS tiles where legal: 2 x 2 tiles of 64 (13 rows, 8 / 36 columns in the last)",
         claims={"predict": [g(LDS, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS)],
                 "input_grad": [g(LDS, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_SOFTMAX_CE),
                                g(FRAG4, 0, 0, 0, 0, EPI_DZ_INFER), g(LDS, 0, 0, 0, 0, EPI_DZ_INFER), g(LDS, 0, 0, 0, 0, EPI_STORE)],
                 "attack_step": [g(LDS, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_SOFTMAX_CE),
                                 g(FRAG4, 0, 0, 0, 0, EPI_DZ_INFER), g(LDS, 0, 0, 0, 0, EPI_DZ_INFER), g(LDS, 0, 0, 0, 0, EPI_SIGNSTEP)],
                 "output_vjp": [g(LDS, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS_RELU_BN), g(FRAG4, 0, 0, 1, 0, EPI_BIAS),
                                g(FRAG4, 0, 0, 0, 0, EPI_DZ_INFER), g(LDS, 0, 0, 0, 0, EPI_DZ_INFER), g(LDS, 0, 0, 0, 0, EPI_STORE)]}),
]
INFER_SPEC = _spec(W_SMALL, (2,), ())   # layer 2 without BatchNorm: EPI_BIAS_RELU_BN / EPI_DZ_INFER without the BatchNorm factors
SOLID = 1e-4  # a gradient component counts where |g| > SOLID max |g|: the cut of test_attacks_gpu.py, twice the 5e-5 the gradient is held to


@functools.lru_cache(maxsize=None)
def _infer_reference():
    # Signed kernels: with the all-positive ones of the training cases, moving statistics that the activations do not follow leave
    # some layer without a live ReLU for 70 % of the rows, and their input gradient is exactly zero.
    spec = INFER_SPEC
    p = _state(spec, 4, nonneg=False)
    rng = np.random.default_rng(82)
    x = rng.standard_normal((77, W_SMALL[0])).astype(np.float32)
    y = P.to_categorical(rng.integers(0, 10, 77), 10)
    p64, x64, y64 = p.astype(np.float64), x.astype(np.float64), y.astype(np.float64)
    v = rng.standard_normal(y.shape).astype(np.float32)
    gx = P.input_gradient_infer(spec, p64, x64, y64)
    vjp, _ = P.output_vjp_infer(spec, p64, x64, v.astype(np.float64))
    return dict(p=p, x=x, y=y, prob=P.forward_infer(spec, p64, x64), gx=gx, v=v, vjp=vjp, solid=np.abs(gx) > SOLID * np.abs(gx).max())


def test_inference_reference_is_decisive():
    """(no GPU) The sign-step comparison leaves out components whose float64 gradient is within fp32 noise of zero: under 1 %."""
    assert _infer_reference()["solid"].mean() > 0.99


@gpu
@pytest.mark.parametrize("case", INFER_CASES, ids=[c["id"] for c in INFER_CASES])
def test_inference_epilogues_against_float64_oracle(cuda, case):
    """predict, input_grad, attack_step (norm inf) and output_vjp on W_SMALL at batch 77 against the oracle's inference functions:
    EPI_BIAS_RELU_BN, EPI_BIAS, EPI_DZ_INFER, EPI_STORE and EPI_SIGNSTEP on ragged tiles, at the bounds of test_attacks_gpu.py
    (probabilities 2e-5 absolute; gradients 5e-5 and 2e-5 of their maximum; the sign step equal wherever the float64 gradient is
    above fp32 noise)."""
    N = _native()
    ref = _infer_reference()
    spec, p, x, y = INFER_SPEC, ref["p"], ref["x"], ref["y"]
    m = _model(spec, 77, 0, 0, 0, 0, case["knob"])
    load_params(m, p)
    xt, yt, vt = dev(x), dev(y), dev(ref["v"])
    base = (m._plan, N.ptr(m._params), N.ptr(m._bnstate))

    def counted(name, fn):
        before = _snapshot()
        out = fn()
        torch.cuda.synchronize()
        moved = _moved(before, _snapshot())
        missing = set(case["claims"][name]) - set(moved)
        assert not missing, (name, "claimed but did not run", sorted(_key_name(k) for k in missing))
        return out

    prob = counted("predict", lambda: m.predict_device(xt)).cpu().numpy()
    np.testing.assert_allclose(prob, ref["prob"], rtol=0, atol=2e-5)
    gx = torch.full_like(xt, float("nan"))
    counted("input_grad", lambda: N.check(N.lib.lipasr_mlp_input_grad(*base, N.ptr(xt), N.ptr(yt), 77, N.ptr(gx), N.stream_ptr())))
    assert rel_err(gx.cpu().numpy(), ref["gx"]) < 5e-5
    alpha, eps = np.float32(0.1), np.float32(0.25)
    x0 = x + (0.2 * np.random.default_rng(12).uniform(-1, 1, x.shape)).astype(np.float32)  # the ball's centre: some steps leave the ball and are clipped
    xa, x0t = xt.clone(), dev(x0)
    counted("attack_step", lambda: N.check(N.lib.lipasr_mlp_attack_step(*base, N.ptr(xa), N.ptr(x0t), N.ptr(yt), 77, float(alpha), float(eps), N.stream_ptr())))
    want = A.sign_step(x, x0, ref["gx"].astype(np.float32), alpha, eps)
    clipped = np.abs(want - x0) >= eps * (1 - 1e-6)
    assert 0.05 < clipped.mean() < 0.95  # both branches of the clip are exercised
    solid = ref["solid"]
    assert solid.mean() > 0.99
    np.testing.assert_allclose(xa.cpu().numpy()[solid], want[solid], rtol=0, atol=2e-6)  # (a flipped sign would move a component by 2 alpha = 0.2)
    vjp = torch.full_like(xt, float("nan"))
    counted("output_vjp", lambda: N.check(N.lib.lipasr_mlp_output_vjp(*base, N.ptr(xt), N.ptr(vt), 0, 77, None, N.ptr(vjp), N.stream_ptr())))
    assert rel_err(vjp.cpu().numpy(), ref["vjp"]) <= 2e-5


# =================================================================================================
# 4. completeness: every instance the library has is claimed by a case
# =================================================================================================
NOT_REACHED = {}  # key -> one sentence on why no case can reach it


def test_every_instance_is_claimed_by_a_case():
    """(no GPU) The library's own list of instantiated kernels (keys whose counter is not -1) and the grouped variants against the
    claims of the tables above: a kernel added without a case fails here, whatever the order the tests run in."""
    claimed = set()
    for case in PLAIN_CASES + list(PLAN_CASES):
        claimed |= {k if k[0] == "group" else k[:5] for k in case["claims"]}
    for case in INFER_CASES:
        for keys in case["claims"].values():
            claimed |= {k[:5] for k in keys}
    have = set(_instances()) | set(GROUP_KEYS)
    assert len(_instances()) >= 58
    missing = have - claimed - set(NOT_REACHED)
    assert not missing, "no case runs: " + "; ".join(_key_name(k) for k in sorted(missing, key=str))
    assert not (claimed - have), "claimed but not in the library: " + "; ".join(_key_name(k) for k in sorted(claimed - have, key=str))
    assert not (set(NOT_REACHED) & claimed), "listed as not reached, yet claimed"
