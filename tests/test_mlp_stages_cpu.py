"""The references and bounds of tests/mlp_stage_ref.py are right and decisive (no GPU needed):

  * every reference agrees with the float64 oracle (oracle/mlp_ref.forward_backward, train_step, adam_update, output_vjp_infer);
  * a float32 restatement of every stage, in the kernel's order, stays inside the stage's bound on the inputs of
    test_mlp_stages_gpu.py -- every element, no share;
  * every mutant exceeds the bound on those inputs.  Where a mutant cannot be told from the reference on one case, the test says so
    and names the case that catches it (ADAM_BLIND: the two mutants that live in lr_t vanish at t = 100000; t = 0, 1, 9 catch them).

The BatchNorm inputs of the GPU file are the device's own activations; here they are the float32 NumPy product of the same x, W, b
(the same values to GEMM rounding).
"""
import numpy as np
import pytest

import mlp_stage_ref as R
from oracle import mlp_ref as P

SMALL = R.ADAM_MODELS["nonneg-layer-0"]      # widths, bn, nonneg
SMALL_NN1 = R.ADAM_MODELS["nonneg-layer-1"]  # NonNeg on layer 1 only


def _frac(got, ref, bound):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / bound


# ====================================================================================================== oracle agreement
def _oracle_model(seed=0):
    rng = np.random.default_rng(seed)
    spec = [P.LayerSpec(6, 9, True, 0.25, True), P.LayerSpec(9, 4, False, 0.0, False)]
    p = P.init_params(spec, seed=seed, dtype=np.float64)
    p.b[0] = 0.1 * rng.standard_normal(9); p.gamma[0] = rng.uniform(0.5, 1.5, 9); p.beta[0] = 0.2 * rng.standard_normal(9)
    p.mov_mean[0] = 0.1 * rng.standard_normal(9); p.mov_var[0] = rng.uniform(0.5, 2.0, 9)
    x = rng.standard_normal((13, 6))
    y = np.eye(4)[rng.integers(0, 4, 13)]
    mask = R.dropout_masks(13, 9, 0.25, seed).astype(np.float64)
    return spec, p, x, y, mask


def test_batchnorm_references_agree_with_the_oracle():
    spec, p, x, y, mask = _oracle_model()
    out = P.forward_backward(spec, p, x, y, masks=[mask, None])
    B = x.shape[0]
    a = np.maximum(x @ p.W[0] + p.b[0], 0)
    # float32 containers are the references' interface: feed float64 through them by checking at float32 resolution
    st = R.bn_stats(a.astype(np.float32), p.mov_mean[0], p.mov_var[0])
    np.testing.assert_allclose(st["mean"], out["stats"][0][0], rtol=3e-7, atol=1e-7)
    np.testing.assert_allclose(st["var"], out["stats"][0][1], rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(st["rstd"], 1 / np.sqrt(out["stats"][0][1] + P.BN_EPS), rtol=3e-6)
    q = p.copy()
    P.train_step(spec, q, P.AdamState(), x, y, masks=[mask, None])
    np.testing.assert_allclose(st["mmean"], q.mov_mean[0], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(st["mvar"], q.mov_var[0], rtol=1e-6, atol=1e-7)
    H, _ = R.bn_apply(a, st["mean"], st["rstd"], p.gamma[0], p.beta[0], mask)
    logits = H @ p.W[1] + p.b[1]
    np.testing.assert_allclose(logits, out["logits"], rtol=1e-5, atol=1e-5)
    s = R.softmax_ce(out["logits"].astype(np.float32), y, 1.0 / B)
    np.testing.assert_allclose(s["p"], out["prob"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(s["loss"].mean(), out["loss"], rtol=1e-5)
    g, _ = R.g_from_next_layer((out["prob"] - y) / B, p.W[1], mask)
    dbeta, dgamma, _, _ = R.bn_bwd_sums(g, a, st["mean"], st["rstd"])
    np.testing.assert_allclose(dbeta, out["dbeta"][0], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(dgamma, out["dgamma"][0], rtol=1e-5, atol=1e-7)
    dz, _ = R.bn_bwd_dz(g, a, st["mean"], st["rstd"], p.gamma[0], dbeta, dgamma, B)
    np.testing.assert_allclose(x.T @ dz, out["dW"][0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dz.sum(axis=0), out["db"][0], rtol=1e-4, atol=1e-6)


def test_adam_reference_agrees_with_the_oracle():
    rng = np.random.default_rng(3)
    hp = R.ADAM_HP
    for t_word in R.ADAM_T:
        w, g, m, v = (rng.standard_normal(257).astype(np.float32) for _ in range(4))
        v = np.abs(v)
        clamp = rng.random(257) < 0.5
        ref = R.adam(w, g, m, v, t_word, gscale=1.0, clamp=clamp, **hp)
        wo, mo, vo = w.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
        P.adam_update(wo, g.astype(np.float64), mo, vo, t_word + 1, lr=R.f32(hp["lr"]), b1=R.f32(hp["b1"]), b2=R.f32(hp["b2"]), eps=R.f32(hp["eps"]))
        wo = np.where(clamp, wo * (wo >= 0), wo)
        for k, o in (("w", wo), ("m", mo), ("v", vo)):
            np.testing.assert_allclose(ref[k], o, rtol=1e-12, atol=1e-300)
    # a whole training step of the oracle: every trainable tensor, NonNeg on the constrained kernel, t = 1
    spec, p, x, y, mask = _oracle_model(1)
    q = p.copy()
    out = P.train_step(spec, q, P.AdamState(), x, y, masks=[mask, None])
    for name, before, after, grad, clamp in (("W0", p.W[0], q.W[0], out["dW"][0], True), ("b0", p.b[0], q.b[0], out["db"][0], False),
                                             ("gamma0", p.gamma[0], q.gamma[0], out["dgamma"][0], False), ("W1", p.W[1], q.W[1], out["dW"][1], False)):
        b32, g32 = before.astype(np.float32), grad.astype(np.float32)
        z = np.zeros_like(b32)
        ref = R.adam(b32, g32, z, z, 0, gscale=1.0, clamp=np.full(b32.shape, clamp), **dict(hp, lr=P.ADAM_LR, b1=P.ADAM_B1, b2=P.ADAM_B2, eps=P.ADAM_EPS))
        # (the oracle starts from the float64 tensors: compare the steps, which the float32 containers round at 1e-7 relative)
        hit = clamp & (after == 0)  # where the oracle's NonNeg acted the reference gives exactly 0 as well; elsewhere the same step
        assert (ref["w"][hit] == 0).all() and (ref["w"][~hit] != 0).all() and (not clamp or hit.any()), name
        np.testing.assert_allclose((ref["w"] - b32)[~hit], (after - before)[~hit], rtol=2e-5, atol=1e-9, err_msg=name)


def test_softmax_vjp_reference_agrees_with_the_oracle():
    rng = np.random.default_rng(5)
    C = 6
    spec = [P.LayerSpec(C, C, False, 0.0, False)]
    p = P.Params(W=[np.eye(C)], b=[np.zeros(C)], gamma=[None], beta=[None], mov_mean=[None], mov_var=[None])
    z = (2.0 * rng.standard_normal((9, C))).astype(np.float32)
    v = rng.standard_normal((9, C)).astype(np.float32)
    for on_logits in (False, True):
        dx, prob = P.output_vjp_infer(spec, p, z.astype(np.float64), v.astype(np.float64), on_logits=on_logits)
        dz, _, pr, _ = R.softmax_vjp(z, v, on_logits)
        np.testing.assert_allclose(dz, dx, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(pr, prob, rtol=1e-12)
    g = P.input_gradient_infer(spec, p, z.astype(np.float64), np.eye(C)[rng.integers(0, C, 9)])
    assert g.shape == z.shape


# ====================================================================================================== Adam: restatement and mutants
def _adam_case(model, seed=R.ADAM_SEED):
    widths, bn, nonneg = model
    segs, n = R.segments(widths, bn, nonneg)
    return segs, n, R.adam_inputs(segs, n, seed), R.clamp_mask(segs, n)


def test_segments_restates_the_layout():
    import lipasr._native as N

    for widths, bn, nonneg in (SMALL, SMALL_NN1, ((1500, 1500, 10), (0, 0), (1, 1))):
        segs, n = R.segments(widths, bn, nonneg)
        lay, po, _ = N.bounds_layout(widths, list(bn) + [0])
        assert n == po
        assert [s[2] for s in segs if s[0] == "W"] == [d["W"] for d in lay] and [s[2] for s in segs if s[0] == "b"] == [d["b"] for d in lay]
    segs, n = R.segments(*SMALL)
    assert [(s[0], s[2], s[3]) for s in segs] == [("W", 0, 35), ("b", 36, 7), ("gamma", 44, 7), ("beta", 52, 7), ("W", 60, 21), ("b", 84, 3)] and n == 88
    assert (2_270_000 >> 2) > 2048 * 256 and R.segments((1500, 1500, 10), (0, 0), (1, 1))[1] > 4 * 2048 * 256  # the stride loop's second trip


@pytest.mark.parametrize("model", [SMALL, SMALL_NN1], ids=["nonneg-layer-0", "nonneg-layer-1"])
@pytest.mark.parametrize("gscale", R.ADAM_GSCALE)
@pytest.mark.parametrize("t_word", R.ADAM_T)
def test_adam_float32_restatement_inside_the_bound(model, t_word, gscale):
    segs, n, (w, g, m, v), clamp = _adam_case(model)
    ref = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, **R.ADAM_HP)
    got = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, dtype=np.float32, **R.ADAM_HP)
    for k, b in (("w", "bw"), ("m", "bm"), ("v", "bv")):
        assert _frac(got[k], ref[k], ref[b]).max() <= 1.0, (k, _frac(got[k], ref[k], ref[b]).max())
    live = R.live_mask(segs, n)
    assert (got["w"][~live] == 0).all() and (got["m"][~live] == 0).all() and (got["v"][~live] == 0).all()
    for _, _, s, c, cl in segs:
        if c >= 6:
            assert got["w"][s] == w[s] and got["w"][s + 1] == 0 and not np.signbit(got["w"][s + 1]) and np.signbit(got["w"][s + 2])
            assert (got["w"][s + 3] == 0) if cl else (got["w"][s + 3] < 0)


def test_adam_float32_restatement_inside_the_bound_large_random():
    """the distribution alone, 2^20 elements per (t, gscale): no special rows, every clamp rule"""
    rng = np.random.default_rng(0)
    n = 1 << 20
    segs = [("W", 0, 0, n, True)]
    for t_word in R.ADAM_T:
        for gscale in R.ADAM_GSCALE:
            w, g, m, v = R.adam_inputs(segs, n, int(rng.integers(1 << 30)))
            # the inputs are the distribution: most of g, m and v are non-zero and span the decades the docstring names
            for a, lo, hi in ((g, 1e-11, 1e2), (m, 1e-11, 1e2), (v, 1e-22, 1e5)):
                assert 0.8 < (a != 0).mean() < 0.95 and np.abs(a[a != 0]).min() < lo and np.abs(a).max() > hi
            clamp = rng.random(n) < 0.5
            ref = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, **R.ADAM_HP)
            got = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, dtype=np.float32, **R.ADAM_HP)
            for k, b in (("w", "bw"), ("m", "bm"), ("v", "bv")):
                assert _frac(got[k], ref[k], ref[b]).max() <= 1.0, (t_word, gscale, k)


STRIDE_LOOP = R.ADAM_MODELS["stride-loop"]
STRIDE_LOOP_CASES = R.ADAM_STRIDE_LOOP_CASES


@pytest.mark.parametrize("t_word,gscale", STRIDE_LOOP_CASES, ids=[f"t{t}" for t, _ in STRIDE_LOOP_CASES])
def test_adam_float32_restatement_inside_the_bound_stride_loop_plan(t_word, gscale):
    """the inputs of the GPU file's 2.27 M-parameter plan (same segments, same seed)"""
    segs, n, (w, g, m, v), clamp = _adam_case(STRIDE_LOOP)
    assert (n >> 2) > 2048 * 256 and (g != 0).mean() > 0.8 and clamp[R.live_mask(segs, n)].mean() > 0.99
    ref = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, **R.ADAM_HP)
    got = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, dtype=np.float32, **R.ADAM_HP)
    for k, b in (("w", "bw"), ("m", "bm"), ("v", "bv")):
        assert _frac(got[k], ref[k], ref[b]).max() <= 1.0, (k, _frac(got[k], ref[k], ref[b]).max())


@pytest.mark.parametrize("wrong", R.ADAM_MUTANTS)
def test_adam_mutants_exceed_the_bound(wrong):
    segs, n, (w, g, m, v), clamp = _adam_case(SMALL)
    live = R.live_mask(segs, n)
    caught = []
    for t_word in R.ADAM_T:
        for gscale in R.ADAM_GSCALE:
            if wrong == "gscale_once" and gscale == 1.0:
                continue  # g'^2 = g^2 gscale when gscale = 1: the cases with gscale 0.5 and 1/3 catch it
            ref = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, **R.ADAM_HP)
            bad = R.adam(w, g, m, v, t_word, gscale=gscale, clamp=clamp, dtype=np.float32, wrong=wrong, **R.ADAM_HP)
            fr = np.maximum(_frac(bad["w"], ref["w"], ref["bw"]), np.maximum(_frac(bad["m"], ref["m"], ref["bm"]), _frac(bad["v"], ref["v"], ref["bv"])))[live]
            if (wrong, t_word) in R.ADAM_BLIND:
                # b^t has vanished: lr_t and eps sqrt(1 - b2^t) are the reference's to rounding.  t = 0, 1, 9 (and 999 for b2) catch it.
                assert fr.max() <= 1.0
                continue
            assert fr.max() > 1.0 and (fr > 1.0).mean() > 0.05, (wrong, t_word, gscale, fr.max(), (fr > 1.0).mean())
            caught.append((t_word, gscale))
    assert caught


def test_adam_clamp_on_the_wrong_segment_exceeds_the_bound():
    for model, other in ((SMALL, SMALL_NN1), (SMALL_NN1, SMALL)):
        segs, n, (w, g, m, v), clamp = _adam_case(model)
        wrong_clamp = R.clamp_mask(*R.segments(*other))
        ref = R.adam(w, g, m, v, 0, gscale=1.0, clamp=clamp, **R.ADAM_HP)
        bad = R.adam(w, g, m, v, 0, gscale=1.0, clamp=wrong_clamp, dtype=np.float32, **R.ADAM_HP)
        fr = _frac(bad["w"], ref["w"], ref["bw"])
        for name, _, s, c, cl in segs:
            if name == "W":
                assert fr[s:s + c].max() > 1.0, "both kernels hold negative updates: each rule is told from the other"


# ====================================================================================================== BatchNorm
def _bn_case(N, B, masked=True):
    mdl = R.bn_model(R.BN_N_IN, N, R.BN_C, B)
    q = np.float32
    A = np.maximum(mdl["x"] @ mdl["W0"] + mdl["b0"], q(0))
    mask = R.dropout_masks(B, N, R.BN_RATE, N + B) if masked else None
    dz1 = ((np.random.default_rng(N * B).standard_normal((B, R.BN_C)) * 0.3 / B)).astype(q)
    g = ((dz1 @ mdl["W1"].T) * (1 if mask is None else mask)).astype(q)
    return mdl, A, mask, g


@pytest.mark.parametrize("shape", list(R.BN_SHAPES), ids=lambda s: f"N{s[0]}-B{s[1]}")
def test_batchnorm_float32_restatement_inside_the_bound(shape):
    N, B = shape
    mdl, A, mask, g = _bn_case(N, B)
    assert (A[:, 0] == 0).all() and (N < 2 or (A[:, 1] == np.float32(0.75)).all())
    if N > 2 and B >= 7:
        assert 30 < A[:, 2].mean() / A[:, 2].std() < 300
    ref = R.bn_stats(A, mdl["mmean"], mdl["mvar"])
    got = R.bn_stats(A, mdl["mmean"], mdl["mvar"], dtype=np.float32)
    for k in ("mean", "var", "rstd", "mmean", "mvar"):
        assert _frac(got[k], ref[k], ref["b_" + k]).max() <= 1.0, k
    mean, rstd = got["mean"], got["rstd"]  # the later stages are fed the (float32) statistics of the implementation under test
    H, bH = R.bn_apply(A, mean, rstd, mdl["gamma"], mdl["beta"], mask)
    H32, _ = R.bn_apply(A, mean, rstd, mdl["gamma"], mdl["beta"], mask, dtype=np.float32)
    assert _frac(H32, H, bH).max() <= 1.0 and (H32[mask == 0] == 0).all()
    db, dg, bdb, bdg = R.bn_bwd_sums(g, A, mean, rstd)
    db32, dg32, _, _ = R.bn_bwd_sums(g, A, mean, rstd, dtype=np.float32)
    assert _frac(db32, db, bdb).max() <= 1.0 and _frac(dg32, dg, bdg).max() <= 1.0
    dz, bdz = R.bn_bwd_dz(g, A, mean, rstd, mdl["gamma"], db32, dg32, B)
    dz32, _ = R.bn_bwd_dz(g, A, mean, rstd, mdl["gamma"], db32, dg32, B, dtype=np.float32)
    assert _frac(dz32, dz, np.maximum(bdz, R.TINY)).max() <= 1.0 and (dz32[A <= 0] == 0).all()


@pytest.mark.parametrize("wrong", R.BN_MUTANTS)
def test_batchnorm_mutants_exceed_the_bound(wrong):
    caught, blind = [], []
    for N, B in R.BN_SHAPES:
        mdl, A, mask, g = _bn_case(N, B)
        ref = R.bn_stats(A, mdl["mmean"], mdl["mvar"])
        if wrong in ("sample_var", "mom_batch", "eps_out"):
            bad = R.bn_stats(A, mdl["mmean"], mdl["mvar"], dtype=np.float32, wrong=wrong)
            keys = {"sample_var": ("var", "rstd", "mvar"), "mom_batch": ("mmean", "mvar"), "eps_out": ("rstd",)}[wrong]
            fr = max(_frac(bad[k], ref[k], ref["b_" + k]).max() for k in keys)
        else:
            mean, rstd = ref["mean"].astype(np.float32), ref["rstd"].astype(np.float32)
            db, dg, _, _ = R.bn_bwd_sums(g, A, mean, rstd)
            dz, bdz = R.bn_bwd_dz(g, A, mean, rstd, mdl["gamma"], db, dg, B)
            bad, _ = R.bn_bwd_dz(g, A, mean, rstd, mdl["gamma"], db, dg, B, dtype=np.float32, wrong=wrong)
            fr = _frac(bad, dz, np.maximum(bdz, R.TINY)).max()
        if wrong in ("sample_var", "no_rstd", "no_dgamma") and B == 1:
            # one row: the variance is 0 under either divisor, and dz = gamma rstd (g - g - 0) is 0 with or without rstd and the
            # dgamma term; every other batch size catches these three
            assert fr <= 1.0
            blind.append((N, B))
            continue
        assert fr > 1.0, (wrong, N, B, fr)
        caught.append((N, B))
    assert len(caught) >= len(R.BN_SHAPES) - 1


def test_exchange_path_g_bound_covers_a_float32_product():
    for N, B in R.BN_SHAPES:
        mdl, A, mask, _ = _bn_case(N, B)
        dz1 = (np.random.default_rng(1).standard_normal((B, R.BN_C)) / B).astype(np.float32)
        g, dg = R.g_from_next_layer(dz1, mdl["W1"], mask)
        g32 = np.zeros((B, N), np.float32)
        for k in range(R.BN_C):
            g32 = g32 + dz1[:, k:k + 1] * mdl["W1"][:, k][None, :]
        g32 = g32 * mask
        assert _frac(g32, g, dg).max() <= 1.0


# ====================================================================================================== softmax
SOFTMAX_SHAPES = [(C, B) for C in (1, 2, 10, 32) for B in (1, 255, 257)]


@pytest.mark.parametrize("shape", SOFTMAX_SHAPES, ids=lambda s: f"C{s[0]}-B{s[1]}")
def test_softmax_float32_restatement_inside_the_bound(shape):
    C, B = shape
    z, y = R.softmax_rows(C, B)
    ref = R.softmax_ce(z, y, 1.0 / B)
    got = R.softmax_ce(z, y, 1.0 / B, dtype=np.float32)
    assert np.isfinite(ref["loss"]).all() and np.isfinite(got["loss"]).all()
    for k in ("p", "loss", "dz"):
        assert _frac(got[k], ref[k], ref["b_" + k]).max() <= 1.0, k
    for k in ("am", "ay", "correct", "onehot"):
        assert np.array_equal(got[k], ref[k])
    if C > 1 and B > 4:
        np.testing.assert_allclose(ref["loss"][4], 200.0, rtol=1e-6)  # the spread of 200 with the label on an underflowed class
    v = np.random.default_rng(C + B).standard_normal((B, C)).astype(np.float32)
    dz, bound, _, _ = R.softmax_vjp(z, v, False)
    dz32, _, _, _ = R.softmax_vjp(z, v, False, dtype=np.float32)
    assert _frac(dz32, dz, bound).max() <= 1.0
    for cls in range(C):
        e = np.zeros((B, C), np.float32); e[:, cls] = 1.0
        dz, bound, _, _ = R.softmax_vjp(z, e, False)
        assert _frac(R.softmax_vjp(z, e, False, dtype=np.float32)[0], dz, bound).max() <= 1.0


@pytest.mark.parametrize("wrong", R.SOFTMAX_MUTANTS)
def test_softmax_mutants_exceed_the_bound(wrong):
    caught = []
    for C, B in SOFTMAX_SHAPES:
        z, y = R.softmax_rows(C, B)
        ref = R.softmax_ce(z, y, 1.0 / B)
        bad = R.softmax_ce(z, y, 1.0 / B, dtype=np.float32, wrong=wrong)
        if wrong == "last_tie":
            hit = not (np.array_equal(bad["am"], ref["am"]) and np.array_equal(bad["ay"], ref["ay"]) and np.array_equal(bad["onehot"], ref["onehot"]))
            if C == 1 or B < 3:
                assert not hit  # one class has no tie, and a batch of one holds only the random row: C >= 2 with B >= 255 catch it
                continue
        else:
            with np.errstate(all="ignore"):
                hit = not (_frac(bad["loss"], ref["loss"], ref["b_loss"]) <= 1.0).all()
            if C == 1 or B < 5:
                continue  # log p = zs - lse to rounding while p is a normal number: the spread-200 row (row 4, C >= 2) catches it
        assert hit, (wrong, C, B)
        caught.append((C, B))
    assert caught
