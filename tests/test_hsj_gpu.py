"""HopSkipJump on the MI355X: the four kernels against their host twins (which tests/test_hsj_cpu.py pins against the NumPy
restatement) at the same shapes and at buffer offsets 0 and 1, on hand-made logits; and the attack's properties on the SMALL model of
test_square_gpu.py, on a linear two-class model and on a small WaveformClassifier with clips of 16 000, 9 000, 37 and 0 samples.

Bounds.  Bits: expand in L-inf; both sums and both counts of accumulate, one call and split 1 + 2 + rest; direction in L-inf; every
state array of search after every call in all three modes.  One unit in the last place of float32: direction in L2 and the two L2
distances (an fp64 tree against the twin's serial sum: n 2^-52 relative) -- the twin restarts from the device's state before every
call, so such a difference never feeds a later decision.  expand in L2: the device's logf / sinf / cosf are not the host's, so the
comparison is with the float64 restatement, bound 8 x the worst error of the float32 NumPy restatement against that same float64
one, the worst taken over the cases of the shape (the form of test_psycho_gpu.py, no floor); measured at these shapes: device
2.8e-9 (n = 1) to 6.0e-8 (n = 22 050), the float32 restatement the same figures to the digits printed, bounds 2.2e-8 to 4.8e-7.
The L-inf comparison runs again at 4 096, 4 099, 8 192, 16 000, 24 576, 24 579 and 24 580 elements, so that every instance of the
expand kernel, the one for wide rows included, is launched.

The linear model (test_hsj_cpu.linear_model: sign(w x + b), true distance |w x + b| / ||w||_2 or / ||w||_1).  n = 36, 12 rows,
max_iter 10, init_eval 100, max_eval 1000.  The restatement, with the device's own counters, reaches R = 1.0208 (L2) and 1.0812
(L-inf) at worst over those rows (test_hsj_cpu.test_restatement_on_a_linear_model measures and pins them); the device has to stay
within 1 + 2 (R - 1), the factor 2 for one-ulp decisions that send it down another branch, to go below the true distance by no more
than the rounding of the row, n 2^-24 max|x|, and to improve on its start on every row."""
import math

import numpy as np
import pytest
import torch

import hsj_ref as R
import local_lip_ref as L
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P
from test_hsj_cpu import (HSJ_KEY, LIN_KW, LIN_R, LIN_SEED, NORMS, SHAPES, STATE, assert_state, host_search, ids, linear_model,
                          linear_truth, logits_for, n_valid_cases, rows, same, search_script, search_setup, within_one_ulp, workspace)

pytestmark = pytest.mark.gpu


def _place(x, offset=0, fill=0.0):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into its allocation."""
    x = np.asarray(x)
    buf = torch.full((x.size + offset,), fill, device="cuda", dtype=torch.as_tensor(x[:0]).dtype)
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def _i32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()


def _N():
    from lipasr import _native as N

    return N


# =================================================================================================
# 1. the kernels against the host twins
# =================================================================================================
def _expand_cases(shape):
    B, n = shape
    yield 1, None, {}, (0, 0)
    yield 3, None, dict(clip0=5, draw0=2, clip_values=(-0.4, 0.45)), (1, 0)
    yield (100 if n <= 1030 else 5), None, {}, (0, 1)
    for nv, offs in zip(n_valid_cases(B, n), [(1, 1), (0, 0)] * 4):
        yield 3, nv, {}, offs


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_expand_equals_the_host_twin(cuda, shape):
    from lipasr.hopskipjump import hsj_expand

    N = _N()
    B, n = shape
    x = rows(B, n, 1 + n)
    delta = np.linspace(0.05, 0.3, B).astype(np.float32)
    l2_cases = []  # (case, device error, float32 restatement's error), both against the float64 restatement
    for draws, nv, kw, offs in _expand_cases(shape):
        hkw = {k: v for k, v in kw.items() if k != "clip_values"}
        lo, hi = kw.get("clip_values", (-np.inf, np.inf))
        for norm in NORMS:
            out = _place(np.full((B * draws, n), 7.0, dtype=np.float32), offs[1])
            hsj_expand(_place(x, offs[0]), dev(delta), draws, 4, 77, norm, out=out, n_valid=None if nv is None else _i32(nv), **kw)
            got = out.cpu().numpy()
            if norm != 2:
                assert same(got, N.hsj_expand_host(x, delta, draws, 4, 77, norm, n_valid=nv, clip_lo=lo, clip_hi=hi, **hkw)), (shape, draws, nv, offs)
                continue
            if draws > 5:
                continue
            args = (nv, kw.get("clip0", 0), kw.get("draw0", 0), lo, hi)
            want = R.expand(x, delta, draws, 4, 77, 2, *args)
            f32_err = float(np.abs(R.expand(x, delta, draws, 4, 77, 2, *args, dtype=np.float32) - want).max())
            l2_cases.append(((draws, nv, offs), float(np.abs(got - want).max()), f32_err))
            valid = np.broadcast_to((np.arange(n)[None, :] < (np.full(B, n) if nv is None else np.clip(nv, 0, n))[:, None])[:, None], (B, draws, n))
            assert same(got.reshape(B, draws, n)[~valid], np.broadcast_to(x[:, None], (B, draws, n))[~valid]), "padding moved"
    yard = max(c[2] for c in l2_cases)  # the worst error of the float32 restatement over the cases of this shape
    print(f"{ids(shape)} expand L2 against float64: worst device {max(c[1] for c in l2_cases):.3e}, float32 restatement {yard:.3e}, "
          f"bound {8 * yard:.3e}")
    for case, err, _ in l2_cases:
        assert err <= 8 * yard, (shape, case, err, yard)
    # chunks of draws and of clips reproduce one call, in either norm, bit for bit
    for norm in NORMS:
        xt, dt = dev(x), dev(delta)
        whole = hsj_expand(xt, dt, 5, 2, 9, norm, out=torch.empty(B * 5, n, device="cuda"))
        parts = torch.cat([hsj_expand(xt[b:b + 1], dt[b:b + 1], d, 2, 9, norm, out=torch.empty(d, n, device="cuda"), clip0=b, draw0=d0)
                           for b in range(B) for d0, d in ((0, 2), (2, 3))])
        assert torch.equal(whole, parts)
        assert torch.equal(whole, hsj_expand(xt, dt, 5, 2, 9, norm, out=torch.empty(B * 5, n, device="cuda")))  # two runs


# the arms of hsj_expand_instance() that SHAPES leaves out: 4 and 8 quads per thread, 4 in workgroups of 1 024 threads (| 32), the
# last size of 6 quads there, and the wide rows (instance 0) that generate the draw a second time, on 16 bytes and off them;
# n -> lipasr_debug_hsj_path(n, aligned)
WIDE = [(4096, 4 | 64), (4099, 8), (8192, 8 | 64), (16000, 4 | 32 | 64), (24576, 6 | 32 | 64), (24580, 0 | 64), (24579, 0)]


@pytest.mark.parametrize("n,path", WIDE, ids=[str(n) for n, _ in WIDE])
def test_expand_linf_equals_the_host_twin_in_every_instance(cuda, n, path):
    from lipasr.hopskipjump import hsj_expand

    N = _N()
    assert N.lib.lipasr_debug_hsj_path(n, 1) == path
    B, draws = 2, 2
    x = rows(B, n, 1 + n)
    delta = np.array([0.05, 0.3], dtype=np.float32)
    for nv, offs, clip in ((None, (0, 0), (-np.inf, np.inf)), ([n - 1, 5], (0, 0), (-0.4, 0.45)), (None, (1, 1), (-np.inf, np.inf))):
        out = _place(np.full((B * draws, n), 7.0, dtype=np.float32), offs[1])
        kw = {} if clip[0] == -np.inf else dict(clip_values=clip)
        hsj_expand(_place(x, offs[0]), dev(delta), draws, 4, 77, np.inf, out=out, n_valid=None if nv is None else _i32(nv), clip0=3, draw0=1, **kw)
        want = N.hsj_expand_host(x, delta, draws, 4, 77, np.inf, n_valid=nv, clip0=3, draw0=1, clip_lo=clip[0], clip_hi=clip[1])
        assert same(out.cpu().numpy(), want), (n, nv, offs)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_accumulate_and_direction_equal_the_host_twins(cuda, shape):
    from lipasr.hopskipjump import hsj_accumulate, hsj_direction

    N = _N()
    B, n = shape
    x = rows(B, n, 3 + n)
    delta = np.full(B, 0.2, dtype=np.float32)
    for (draws, C, targeted), offs in zip(((1, 2, False), (3, 10, True), (100 if n <= 1030 else 7, 32, False)), ((0, 0), (1, 0), (0, 1))):
        labels = (np.arange(B) % C).astype(np.int32)
        for nv in [None] + (n_valid_cases(B, n) if draws == 3 else []):
            p = N.hsj_expand_host(x, delta, draws, 1, 5, np.inf, n_valid=nv)
            for share in (0.5, 0.0, 1.0):
                z = logits_for(B, draws, C, labels, draws + C, share)
                if share != 0.5:
                    z = np.nan_to_num(z, nan=0.0)
                    z[np.arange(B * draws), np.repeat(labels, draws)] += -50.0 if (share == 1.0) != targeted else 50.0
                hs, hc = workspace(B, n)
                N.hsj_accumulate_host(z, labels, p, x, sums=hs, counts=hc, n_valid=nv, targeted=targeted)
                xt, pt, zt, lab, nvt = _place(x, offs[0]), _place(p, offs[1]), dev(z), _i32(labels), None if nv is None else _i32(nv)
                sums, counts = torch.zeros(B, 2, n, dtype=torch.float64, device="cuda"), torch.zeros(B, 2, dtype=torch.int32, device="cuda")
                hsj_accumulate(zt, lab, pt, xt, sums=sums, counts=counts, n_valid=nvt, targeted=targeted)
                assert same(sums.cpu().numpy(), hs) and same(counts.cpu().numpy(), hc), (shape, draws, C, nv, share)
                if draws >= 3:
                    ss, sc = torch.zeros_like(sums), torch.zeros_like(counts)
                    p3, z3 = pt.view(B, draws, n), zt.view(B, draws, C)
                    for a, b in ((0, 1), (1, 3), (3, draws)):
                        if b > a:
                            hsj_accumulate(z3[:, a:b].reshape(-1, C).contiguous(), lab, p3[:, a:b].reshape(-1, n).contiguous(), xt, sums=ss,
                                           counts=sc, n_valid=nvt, targeted=targeted)
                    assert torch.equal(ss, sums) and torch.equal(sc, counts)
                u = _place(np.full((B, n), 7.0, dtype=np.float32), offs[1])
                hsj_direction(sums, counts, np.inf, u=u, n_valid=nvt)
                assert same(u.cpu().numpy(), N.hsj_direction_host(hs, hc, np.inf, n_valid=nv)), (shape, draws, C, nv, share)
                hsj_direction(sums, counts, 2, u=u, n_valid=nvt)
                assert within_one_ulp(u.cpu().numpy(), N.hsj_direction_host(hs, hc, 2, n_valid=nv)), (shape, draws, C, nv, share)


def _device_search(t, z, s, mode, flags, draw, scale, norm, seed, nvt, clip):
    from lipasr.hopskipjump import hsj_search

    hsj_search(None if z is None else dev(z), t["labels"], t["x0"], mode, flags, seed, norm, x_cand=t["x_cand"], x_far=t["x_far"],
               x_adv=t["x_adv"], x_best=t["x_best"], fstate=t["f"], istate=t["i"], start_lo=t["start_lo"], start_hi=t["start_hi"],
               theta=t["theta"], u=t["u"], n_valid=nvt, clip0=2, draw=draw, step_scale=scale, max_halvings=3,
               clip_values=None if clip[0] == -np.inf else clip, classes=4)


@pytest.mark.parametrize("norm", NORMS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_search_equals_the_host_twin_after_every_call(cuda, shape, norm):
    B, n = shape
    cases = [(None, (-np.inf, np.inf), 0), (None, (-0.5, 0.6), 1)] + [(v, (-1.0, 1.0), k % 2) for k, v in enumerate(n_valid_cases(B, n))]
    for nv, clip, off in cases:
        seed = 21 + n
        s = search_setup(shape, norm, seed, nv, clip=clip)
        st = R.new_state(B, n, s["attack"])
        for k in ("x_cand", "x_far"):
            st[k][:] = 7.0
        t = {k: _place(st[k], off if k in ("x_cand", "x_adv") else 0) for k in STATE}
        t.update(x0=_place(s["x0"], off), u=_place(s["u"], 0), labels=_i32(s["labels"]))
        t.update({k: dev(s[k]) for k in ("start_lo", "start_hi", "theta")})
        nvt = None if nv is None else _i32(nv)
        for step, (mode, flags, draw, z, scale) in enumerate(search_script(B, 4, s["labels"], seed)):
            host = {k: t[k].cpu().numpy().copy() for k in STATE}  # the twin restarts from the device's state
            _device_search(t, z, s, mode, flags, draw, scale, norm, seed, nvt, clip)
            host_search(host, z, s, mode, flags, draw, scale, norm, seed, nv, clip)
            got = {k: t[k].cpu().numpy() for k in STATE}
            assert_state(got, host, norm == 2, f"{ids(shape)} norm {norm} n_valid {nv} offset {off} step {step} mode {mode} flags {flags}")
        assert same(t["x0"].cpu().numpy(), s["x0"]) and same(t["u"].cpu().numpy(), s["u"])


def test_wrappers_refuse_bad_arguments(cuda):
    from lipasr.hopskipjump import hsj_accumulate, hsj_direction, hsj_expand, hsj_search

    x, delta = dev(rows(2, 8, 0)), torch.ones(2, device="cuda")
    out = torch.empty(6, 8, device="cuda")
    z, lab = dev(logits_for(2, 3, 4, [0, 1], 0)), _i32([0, 1])
    sums, counts = torch.zeros(2, 2, 8, dtype=torch.float64, device="cuda"), torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    hsj_expand(x, delta, 3, 1, 0, 2, out=out)
    hsj_accumulate(z, lab, out, x, sums=sums, counts=counts)
    b = {k: torch.empty(2, 8, device="cuda") for k in ("x_cand", "x_far", "x_adv", "x_best", "u")}
    st = dict(fstate=torch.zeros(2, 8, device="cuda"), istate=torch.ones(2, 8, dtype=torch.int32, device="cuda"), start_lo=-delta, start_hi=delta,
              theta=delta)
    search = lambda **kw: hsj_search(kw.pop("z", z[:2].contiguous()), lab, x, kw.pop("mode", R.BISECT), kw.pop("flags", 0), 0, kw.pop("norm", 2),
                                     **{**b, **st, **kw})
    search(mode=R.START, flags=R.FIRST, z=None, classes=4)
    for bad in (lambda: hsj_expand(x, delta, 3, 1, 0, 1, out=out), lambda: hsj_expand(x, delta, 3, 1 << 24, 0, 2, out=out),
                lambda: hsj_expand(x, delta, 3, 1, 0, 2, out=out[:5]), lambda: hsj_expand(x.cpu(), delta, 3, 1, 0, 2, out=out),
                lambda: hsj_expand(x, delta, 3, 1, 0, 2, out=out, clip_values=(1.0, -1.0)), lambda: hsj_expand(x, delta[:1], 3, 1, 0, 2, out=out),
                lambda: hsj_expand(x, delta, 3, 1, 0, 2, out=out, n_valid=lab.long()),
                lambda: hsj_accumulate(z[:5], lab, out, x, sums=sums, counts=counts), lambda: hsj_accumulate(z, lab.long(), out, x, sums=sums, counts=counts),
                lambda: hsj_accumulate(z, lab, out, x, sums=sums.float(), counts=counts), lambda: hsj_accumulate(z, lab, out, x, sums=sums, counts=counts[:1]),
                lambda: hsj_accumulate(dev(logits_for(2, 3, 33, [0, 1], 0)), lab, out, x, sums=sums, counts=counts),
                lambda: hsj_direction(sums, counts, 1, u=b["u"]), lambda: hsj_direction(sums, counts, 2, u=b["u"][:1]),
                lambda: search(norm=1), lambda: search(mode=3), lambda: search(flags=4), lambda: search(max_halvings=0), lambda: search(step_scale=-1.0),
                lambda: search(z=None), lambda: search(x_far=b["x_cand"]), lambda: search(fstate=st["fstate"][:1]), lambda: search(mode=R.HALVE, u=None),
                lambda: search(clip_values=(1.0, 0.0)), lambda: search(z=dev(logits_for(2, 1, 33, [0, 1], 0)))):
        with pytest.raises(ValueError):
            bad()
    hsj_expand(x[:0], delta[:0], 3, 1, 0, 2, out=out[:0])  # nothing to do, nothing written
    torch.cuda.synchronize()


# =================================================================================================
# 2. the attack on small models
# =================================================================================================
SMALL = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
QUICK = dict(max_iter=4, init_eval=20, max_eval=40, init_size=20, verbose=False)


@pytest.fixture(scope="module")
def small(cuda):
    from lipasr.attacks import TensorFlowV2Classifier

    m = build_model(SMALL, max_batch=64)
    load_params(m, L.setup_params(SMALL, 2))
    x = np.random.default_rng(4).standard_normal((7, 36)).astype(np.float32)
    return dict(model=m, x=x, clf=TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,)))


def _check(atk, predict, x, adv, labels, norm, clip=None, valid=None, targeted=False):
    """The exact properties of one call."""
    valid = np.ones(x.shape, dtype=bool) if valid is None else valid
    ok, dist, q = atk.success_.cpu().numpy(), atk.distance_.cpu().numpy(), atk.queries_.cpu().numpy()
    assert ok.dtype == np.bool_ and dist.dtype == np.float32 and q.dtype == np.int64
    assert same(adv[~valid], x[~valid]), "padding moved"
    pred = predict(adv).argmax(axis=1)
    assert ((pred == labels) if targeted else (pred != labels))[ok].all(), "a returned row with success_ is not adversarial"
    assert same(adv[~ok], x[~ok]) and np.isinf(dist[~ok]).all(), "a row without a start must come back bit for bit"
    if clip is not None:
        assert adv[valid].min() >= np.float32(clip[0]) and adv[valid].max() <= np.float32(clip[1])
    again = np.array([R.distance(np.where(valid[b], adv[b], x[b]), x[b], norm) for b in range(len(x))])
    assert within_one_ulp(dist[ok], again[ok].astype(np.float32)), (dist, again)
    return ok, dist, q


@pytest.mark.parametrize("norm", NORMS, ids=ids)
def test_attack_properties_on_the_small_model(small, norm):
    from lipasr.attacks import DeepFool, HopSkipJump

    clf, x = small["clf"], small["x"]
    xt = dev(x)
    predict = lambda a: clf.predict_device(dev(a), logits=True).cpu().numpy()
    own = predict(x).argmax(axis=1)
    atk = HopSkipJump(clf, norm=norm, seed=3, **QUICK)
    assert atk.clip_values is None and atk.seed == HSJ_KEY + 3
    adv = atk.generate_device(xt)
    assert adv.data_ptr() != xt.data_ptr()
    adv = adv.cpu().numpy()
    ok, dist, q = _check(atk, predict, x, adv, own, norm)
    assert ok.all() and (dist > 0).all() and (dist <= atk.start_distance_.cpu().numpy()).all()
    fool = DeepFool(clf, norm=norm)
    d_fool = R.distance(fool.generate_device(xt).cpu().numpy(), x, norm)
    print(f"SMALL, norm {norm}: HopSkipJump {np.round(dist, 4).tolist()} after {q.tolist()} queries; DeepFool {np.round(d_fool, 4).tolist()}")
    # two runs, chunks of 3 and 7 clips, a look at active after every query, a smaller batch_limit: the same bits
    first = (adv, dist, q)
    for kw in (dict(), dict(batch_size=3), dict(batch_size=7, check_every=1), dict(batch_size=2, check_every=3)):
        other = HopSkipJump(clf, norm=norm, seed=3, **QUICK, **kw)
        assert same(other.generate_device(xt).cpu().numpy(), first[0]), kw
        assert same(other.distance_.cpu().numpy(), first[1]) and same(other.queries_.cpu().numpy(), first[2]), kw
    assert not same(HopSkipJump(clf, norm=norm, seed=4, **QUICK).generate(x), adv)
    onehot = np.eye(5, dtype=np.float32)[own]
    for y in (onehot, own):
        assert same(atk.generate(x, y), adv)
    # a row that is wrong when clean comes back untouched, with distance 0 and no query
    wrong = own.copy()
    wrong[0] = (own[0] + 1) % 5
    back = atk.generate(x[:3], wrong[:3])
    assert same(back[0], x[0]) and bool(atk.success_[0]) and float(atk.distance_[0]) == 0.0 and int(atk.queries_[0]) == 0
    assert same(back[1:], adv[1:3])
    # queries_ is what the model was asked: count the rows that go through predict_device, one clip at a time
    calls = []
    real = clf.predict_device
    clf.predict_device = lambda r, **kw: (calls.append(r.shape[0]), real(r, **kw))[1]
    try:
        for b in (1, 4):
            calls.clear()
            one = HopSkipJump(clf, norm=norm, seed=3, check_every=1, **QUICK)
            one.generate_device(xt[b:b + 1])
            assert int(one.queries_[0]) == sum(calls) - 1, "every row but the clean prediction counts"
    finally:
        del clf.predict_device
    # targeted: the start is given and must already be classified as the target
    target = np.roll(own, 1)
    tgt = HopSkipJump(clf, norm=norm, targeted=True, seed=3, **QUICK)
    adv_t = tgt.generate(x, target, x_adv_init=np.roll(x, 1, axis=0))
    ok_t, dist_t, _ = _check(tgt, predict, x, adv_t, target, norm, targeted=True)
    assert ok_t.all() and (dist_t[target == own] == 0).all() and (dist_t[target != own] > 0).all()
    assert (dist_t <= R.distance(np.roll(x, 1, axis=0), x, norm) * (1 + 1e-6)).all()
    with pytest.raises(ValueError):
        tgt.generate(x, target)
    with pytest.raises(ValueError):
        tgt.generate(x, x_adv_init=np.roll(x, 1, axis=0))
    with pytest.raises(ValueError):
        tgt.generate(x, target, x_adv_init=x)
    for bad in (dict(norm=1), dict(max_iter=-1), dict(max_eval=0), dict(init_eval=0), dict(init_size=0), dict(batch_size=0), dict(check_every=0),
                dict(max_halvings=0), dict(gamma=0.0), dict(clip_values=(1.0, -1.0))):
        with pytest.raises(ValueError):
            HopSkipJump(clf, **bad)
    with pytest.raises(ValueError):
        atk.generate_device(xt, lengths=[36] * 7)
    assert atk.generate_device(xt[:0]).shape == (0, 36)
    # a clip range: every returned row lies inside it
    clip = (-1.5, 1.75)
    xc = np.clip(x, *clip)
    boxed = HopSkipJump(clf, norm=norm, seed=3, clip_values=clip, **QUICK)
    _check(boxed, predict, xc, boxed.generate(xc), predict(xc).argmax(axis=1), norm, clip=clip)


@pytest.mark.parametrize("norm", NORMS, ids=ids)
def test_distance_on_a_linear_model(cuda, norm):
    """distance_ against the true distance |w x + b| / ||w|| of sign(w x + b); the module docstring derives the three bounds."""
    from lipasr.attacks import HopSkipJump, TensorFlowV2Classifier

    (W1, b1, W2, b2), w, b = linear_model()
    spec = [P.LayerSpec(36, 2, False, 0.0, False), P.LayerSpec(2, 2, False, 0.0, False)]
    p = P.init_params(spec, seed=0, dtype=np.float32)
    assert p.W[0].shape == W1.shape and p.W[1].shape == W2.shape
    p.W, p.b = [W1, W2], [b1, b2]
    m = build_model(spec, max_batch=1024)
    load_params(m, p)
    clf = TensorFlowV2Classifier(model=m, nb_classes=2, input_shape=(36,))
    x = rows(12, 36, 5)
    atk = HopSkipJump(clf, norm=norm, seed=LIN_SEED[norm], verbose=False, **LIN_KW)
    adv = atk.generate(x)
    predict = lambda a: clf.predict_device(dev(a), logits=True).cpu().numpy()
    ok, dist, q = _check(atk, predict, x, adv, predict(x).argmax(axis=1), norm)
    true = linear_truth(w, b, x, norm)
    start = atk.start_distance_.cpu().numpy()
    bound = 1 + 2 * (LIN_R[norm] - 1)
    print(f"linear, norm {norm}: distance / true {np.round(dist / true, 4).tolist()} (worst {float((dist / true).max()):.4f}, bound {bound:.4f}); "
          f"start / true {np.round(start / true, 2).tolist()}; queries {q.tolist()}")
    assert ok.all()
    assert (dist >= true - 36 * 2.0 ** -24 * np.abs(x).max()).all()
    assert (dist < start).all()
    assert (dist / true <= bound).all()


RAGGED = [16000, 9000, 37, 0]


def test_attack_over_audio_with_lengths(cuda):
    from lipasr.attacks import HopSkipJump, WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, L.setup_params(spec, 3))
    ex = MfccExtractor(16000, 16000, batch_max=32)
    try:
        w = np.asarray(synth_clips(4, seed=31)[0], dtype=np.float32)
        for r, n in enumerate(RAGGED):
            w[r, n:] = 0
        lt = torch.as_tensor(np.array(RAGGED, dtype=np.int32)).to(cuda)
        xt = ex.resample(torch.as_tensor(w).to(cuda).contiguous(), n_valid=lt)
        clf = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
        x = xt.cpu().numpy()
        assert x.shape == (4, 22050)
        pos = [int(math.ceil(n * 22050.0 / 16000.0)) for n in RAGGED]
        valid = np.arange(22050)[None, :] < np.array(pos)[:, None]
        predict = lambda a: clf.predict_device(torch.as_tensor(a).cuda(), logits=True, lengths=lt).cpu().numpy()
        own = predict(x).argmax(axis=1)
        for norm in NORMS:
            atk = HopSkipJump(clf, norm=norm, seed=2, max_iter=2, init_eval=8, max_eval=16, init_size=10, verbose=False)
            assert atk.clip_values == (-1.0, 1.0)  # the estimator's
            adv = atk.generate_device(xt, lengths=lt).cpu().numpy()
            ok, dist, q = _check(atk, predict, x, adv, own, norm, clip=(-1.0, 1.0), valid=valid)
            print(f"audio 4 x 22050 with lengths, norm {norm}: success {ok.tolist()} distance {dist.tolist()} queries {q.tolist()}")
            assert not ok[3] and q[3] == 0, "a clip without samples has nothing to perturb"
            # uniform noise is one class to this model: a clip of that class finds no start in 10 draws and says so
            assert ok[:3].any() and (q[:3] > 0).all() and (q[:3][~ok[:3]] == 10).all()
            for kw in (dict(batch_size=3), dict(batch_size=1, check_every=1)):
                other = HopSkipJump(clf, norm=norm, seed=2, max_iter=2, init_eval=8, max_eval=16, init_size=10, verbose=False, **kw)
                assert same(other.generate_device(xt, lengths=lt).cpu().numpy(), adv), kw
                assert same(other.queries_.cpu().numpy(), q) and same(other.distance_.cpu().numpy(), dist)
    finally:
        ex.close()


# =================================================================================================
# 3. the read-outs
# =================================================================================================
def test_menu_runs_the_hopskipjump_sweep_and_the_radius(cuda, tmp_path, capsys):
    import wave

    from lipasr import attack_eval as V
    from lipasr.attacks import TensorFlowV2Classifier
    from lipasr.extract_features_construct_dataset import compute_mfcc_all_files, get_robustness_radius
    from lipasr.synth import synth_clips

    waves, lab = synth_clips(12, seed=31)
    files = []
    for i in range(12):
        path = tmp_path / f"clip_{i:03d}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(waves[i], -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats = compute_mfcc_all_files(files)
    lab = np.asarray(lab).astype(np.int64) % 10
    lab[-1] = 9  # main() sizes the one-hot labels by the largest test label
    data, noise = tmp_path / "processed", tmp_path / "noise"
    data.mkdir()
    noise.mkdir()
    for name, sl in (("train", slice(0, 4)), ("dev", slice(4, 8)), ("test", slice(8, 12))):
        np.save(data / f"{name}_data.npy", feats[sl])
        np.save(data / f"{name}_label.npy", lab[sl])
    np.save(noise / "test_filenames.npy", np.array(files[8:12]))
    np.save(noise / "test_label.npy", lab[8:12])
    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, L.setup_params(spec, 3))
    h5 = str(tmp_path / "model.h5")
    m.save(h5)
    common = ["--path", str(data) + "/", "--noise-dir", str(noise), "--constrained", h5, "--unconstrained", h5, "--points", "2"]
    base = common + ["--attack", "black", "--kind", "hsj", "--max-iter", "2"]
    capsys.readouterr()
    for extra, norm in (([], "inf"), (["--norm", "2"], "2"), (["--over", "audio"], "inf")):
        grid, acc, stats = V.main(base + extra)
        out = capsys.readouterr().out
        assert len(grid) == 2 and set(acc) == set(stats) == {"constrained", "unconstrained"}
        assert all(len(v) == 2 and 0.0 <= v[1] <= v[0] <= 1.0 for v in acc.values()), acc  # accuracy falls as eps grows
        assert all(set(v) == {"median_distance", "mean_queries"} for v in stats.values())
        assert f"HopSkipJump (norm {norm})" in out and "median distance" in out and "mean queries" in out
    with pytest.raises(ValueError):
        V.main(base + ["--norm", "1"])
    clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
    x = feats[8:12].astype(np.float32)
    res = get_robustness_radius(clf, x, norm=2, found_by="hopskipjump", max_iter=2, init_eval=10, max_eval=20, verbose=False)
    base_res = get_robustness_radius(clf, x, norm=2)
    assert set(res) == set(base_res) and same(res["margin"], base_res["margin"]) and same(res["certified"], base_res["certified"])
    assert res["found"].shape == (4,) and res["flipped"].dtype == np.bool_ and (res["found"][res["flipped"]] >= res["certified"][res["flipped"]]).all()
    print(f"radius: certified {res['certified'].tolist()} hopskipjump {res['found'].tolist()} deepfool {base_res['found'].tolist()}")
    with pytest.raises(ValueError):
        get_robustness_radius(clf, x, found_by="boundary")
    rep = V.radius_report({"unconstrained": m}, feats[:4], feats[4:8], feats[8:], found_by="hopskipjump", max_iter=1, init_eval=5, max_eval=5,
                          verbose=False)
    assert "unconstrained" in rep
