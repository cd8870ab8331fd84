"""The time-warp operator on the MI355X: lipasr_warp_apply / lipasr_warp_param_vjp against the float64 restatement of
tests/warp_ref.py within the DERIVED bounds of tests/test_warp_cpu.py, at buffer offsets 0 and 1 float, with and without lengths;
equal to the host twins bit for bit and the same bits twice; rows that do not reach into each other; launch counts on the reference
shape; lipasr.attacks.TimeWarp against the float64 worst-of-grid driver, its refinement, targets and chunking; and the menu."""
import functools

import numpy as np
import pytest
import torch

import warp_ref as R
from test_warp_cpu import CASES

import lipasr._native as N
import lipasr.keras as KS

pytestmark = pytest.mark.gpu


def _place(a, offset, dtype=torch.float32, fill=0.0):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into a 16-byte aligned allocation."""
    buf = torch.full((a.size + offset + 4,), fill, device="cuda", dtype=dtype)
    view = buf[offset:offset + a.size].view(*a.shape)
    view.copy_(torch.as_tensor(a))
    return view


def _i32(a):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()


def device_apply(x, params, K, lens, offset=0):
    from lipasr.warp import warp_table

    b, n = x.shape
    xt, pt = _place(x, offset), _place(params, offset)
    out = _place(np.full((b * K, n), 7.0, np.float32), offset)
    lt = _i32(lens)
    N.check(N.lib.lipasr_warp_apply(N.ptr(xt), N.ptr(lt), N.ptr(pt), N.ptr(warp_table()), b, K, n, N.ptr(out), N.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_vjp(x, g, params, K, lens, offset=0):
    from lipasr.warp import warp_table

    b, n = x.shape
    xt, gt, pt = _place(x, offset), _place(g, offset), _place(params, offset)
    gp = torch.full((b * K * 3 + 1,), 7.0, device="cuda", dtype=torch.float64)[:b * K * 3].view(b * K, 3)
    N.check(N.lib.lipasr_warp_param_vjp(N.ptr(xt), N.ptr(gt), N.ptr(_i32(lens)), N.ptr(pt), N.ptr(warp_table()), b, K, n, N.ptr(gp),
                                        N.stream_ptr()))
    torch.cuda.synchronize()
    return gp.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(n, nv, K):
    x, lens, params, g = R.grid_case(n, nv, K)
    ref, rows = R.warp_apply(x, params, K, lens, parts=True)
    return ref, rows, R.param_vjp(x, g, params, K, lens)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n,nv,K", CASES)
def test_device_against_float64_and_the_twin(cuda, n, nv, K, offset):
    x, lens, params, g = R.grid_case(n, nv, K)
    ref, rows, (gref, gbound) = reference(n, nv, K)
    out = device_apply(x, params, K, lens, offset)
    worst = 0.0
    for r, row in enumerate(rows):
        v = R.clamp_nv(lens, r // K, n)
        bound = R.out_bound(row, params[r, 2])
        err = np.abs(out[r].astype(np.float64) - ref[r])
        assert np.all(err <= bound), (r, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(out[r, v:] == 0.0)
        worst = max(worst, float((err[:v] / np.maximum(bound[:v], 1e-300)).max()) if v else 0.0)
    gp = device_vjp(x, g, params, K, lens, offset)
    gerr = np.abs(gp - gref)
    assert np.all(gerr <= gbound), (gerr / np.maximum(gbound, 1e-300)).max()
    print(f"n={n} nv={nv} K={K} offset={offset}: worst |out32 - out64| / bound {worst:.3f}, "
          f"worst |gp - gp64| / bound {float((gerr / np.maximum(gbound, 1e-300)).max()):.3f}")
    # the host twin, bit for bit; and the same bits twice
    assert np.array_equal(out, N.warp_apply_host(x, params, K, n_valid=lens))
    assert np.array_equal(gp, N.warp_param_vjp_host(x, g, params, K, n_valid=lens))
    if offset == 0:
        assert np.array_equal(out, device_apply(x, params, K, lens)) and np.array_equal(gp, device_vjp(x, g, params, K, lens))
        # the same lengths given explicitly and through n_valid == NULL
        full = np.full(len(lens), n, dtype=np.int32)
        assert np.array_equal(device_apply(x, params, K, full), device_apply(x, params, K, None))
        assert np.array_equal(device_vjp(x, g, params, K, full), device_vjp(x, g, params, K, None))


def test_rows_do_not_reach_into_each_other(cuda):
    n, K = 2500, 5  # three spans of 1 024, the last one short
    x, lens, params, g = R.grid_case(n, 1700, K)
    out, gp = device_apply(x, params, K, lens), device_vjp(x, g, params, K, lens)
    for b in range(len(x)):  # a clip launched alone
        sl = slice(b * K, (b + 1) * K)
        assert np.array_equal(device_apply(x[b:b + 1], params[sl], K, lens[b:b + 1]), out[sl])
        assert np.array_equal(device_vjp(x[b:b + 1], g[sl], params[sl], K, lens[b:b + 1]), gp[sl])
    # tails past nv filled with 10 x noise are never read
    noisy = x.copy()
    for b, v in enumerate(lens):
        noisy[b, v:] = 10.0 * np.random.default_rng(b).standard_normal(n - v)
    assert np.array_equal(device_apply(noisy, params, K, lens), out) and np.array_equal(device_vjp(noisy, g, params, K, lens), gp)
    # a NaN sample, a NaN triple, a rate of 3.0 and an n_valid of -5 stay in their own rows
    x2, p2, l2 = x.copy(), params.copy(), lens.copy()
    x2[0, 100] = np.nan
    p2[K + 1] = (np.nan, 1.0, 1.0)
    p2[K + 3] = (0.0, 3.0, 1.0)
    l2 = np.array([lens[0], lens[1], -5], dtype=np.int32)
    out2, gp2 = device_apply(x2, p2, K, l2), device_vjp(x2, g, p2, K, l2)
    assert np.isnan(out2[:K]).any() and np.isnan(out2[K + 1, :lens[1]]).all() and np.isnan(out2[K + 3, :lens[1]]).all()
    assert np.isnan(gp2[K + 1]).all() and np.isnan(gp2[K + 3]).all()
    assert np.all(out2[2 * K:] == 0.0) and np.all(gp2[2 * K:] == 0.0)
    for r in (K, K + 2, K + 4):
        assert np.array_equal(out2[r], out[r]) and np.array_equal(gp2[r], gp[r])
    assert np.array_equal(out2, N.warp_apply_host(x2, p2, K, n_valid=l2), equal_nan=True)


def test_one_launch_per_call_on_the_reference_shape(cuda):
    from lipasr.warp import candidate_grid, warp_apply, warp_param_vjp

    x = torch.randn(4, 22050, device="cuda")
    params = np.tile(candidate_grid(220.5, 1.07, 3.0, counts=(3, 3, 3)), (4, 1))
    before = [N.lib.lipasr_debug_warp_launches(k) for k in (0, 1)]
    rows = warp_apply(x, params, 27)
    assert [N.lib.lipasr_debug_warp_launches(k) for k in (0, 1)] == [before[0] + 1, before[1]]
    gp = warp_param_vjp(x, torch.randn_like(rows), params, 27)
    assert [N.lib.lipasr_debug_warp_launches(k) for k in (0, 1)] == [before[0] + 1, before[1] + 1]
    torch.cuda.synchronize()
    assert rows.shape == (108, 22050) and gp.shape == (108, 3) and bool(torch.isfinite(rows).all()) and bool(torch.isfinite(gp).all())
    assert torch.equal(rows[13::27], x)  # the identity candidate


# ------------------------------------------------------------------------------------------------------------------ the attack
def build(m, max_batch=128):
    """The lipasr.keras.Model of a bounds_ref model, through the layer protocol."""
    KS.reset_layer_names()
    inp = KS.Input((m["widths"][0],))
    node = inp
    L = len(m["W"])
    for l in range(L):
        node = KS.Dense(m["widths"][l + 1], activation="softmax" if l + 1 == L else "relu")(node)
    model = KS.Model(inputs=inp, outputs=node, max_batch=max_batch)
    model.compile(optimizer="adam", loss=KS.CategoricalCrossentropy(), metrics=["accuracy"])
    for l, layer in enumerate(x for x in model.layers if "dense" in x.name):
        layer.set_weights([m["W"][l], m["b"][l]])
    return model


@pytest.fixture(scope="module")
def bed(cuda):
    from lipasr import attacks as A
    from lipasr.extract_features_construct_dataset import MfccExtractor

    m = R.model()
    model = build(m)
    ex = {bm: MfccExtractor(R.SR16, R.N_SAMP, batch_max=bm) for bm in (64, 32)}
    est = {bm: A.WaveformClassifier(model, R.WIDTHS[-1], extractor=e, utterance_length=R.UTT, domain="22k") for bm, e in ex.items()}
    x, lengths = R.clips()
    y = R.own_labels(m, x, lengths)
    yield dict(m=m, est=est[64], est32=est[32], x=x, lengths=lengths, y=y, xt=torch.as_tensor(x).cuda())
    for e in ex.values():
        e.close()


def _left_out(ms, zs):
    """Rows whose float64 answer the device may miss: the best two candidate margins, or the best margin and zero, closer than the
    logit tolerance of the wave-attack tests (1e-3 of the largest logit)."""
    tol = 1e-3 * np.abs(zs).max(axis=(1, 2))
    srt = np.sort(ms, axis=1)
    second = srt[:, 1] if ms.shape[1] > 1 else np.full(len(ms), np.inf)
    return (second - srt[:, 0] < tol) | (np.abs(srt[:, 0]) < tol)


@pytest.mark.parametrize("targeted", [False, True])
def test_time_warp_against_the_float64_driver(bed, targeted):
    from lipasr import attacks as A
    from lipasr.square import margin_device
    from lipasr.warp import candidate_grid, warp_apply

    est, x, lengths, xt = bed["est"], bed["x"], bed["lengths"], bed["xt"]
    y = (bed["y"] + 1) % R.WIDTHS[-1] if targeted else bed["y"]
    atk = A.TimeWarp(est, 256.0, counts=(9, 1, 1), targeted=targeted)
    pick, ms, zs = R.worst_of_grid(bed["m"], x, lengths, atk.grid, y, targeted)
    adv = atk.generate_device(xt, torch.as_tensor(y), lengths=lengths)
    out = _left_out(ms, zs)
    keep = ~out
    print(f"targeted={targeted}: {int(out.sum())} of {len(x)} rows left out; float64 flips {int((ms.min(axis=1) < 0).sum())}, "
          f"device flips {int((atk.margins_ < 0).sum())}")
    assert out.sum() <= 0.1 * len(x)
    grid = atk.grid.astype(np.float32).astype(np.float64)
    got = atk.params_.cpu().numpy()
    assert np.array_equal(got[keep], grid[pick][keep])
    assert np.array_equal((atk.margins_.cpu().numpy() < 0)[keep], (ms.min(axis=1) < 0)[keep])
    if targeted:
        assert (ms.min(axis=1) < 0)[keep].any()  # the reference moves a row to its target, and so did the device
    nv = est.clip_positions(est.lengths_device(lengths, len(x))).to(torch.int32).contiguous()
    assert torch.equal(adv, warp_apply(xt, atk.params_, 1, lengths=nv))
    assert np.all(np.abs(got[:, 0]) <= 256.0) and np.all(got[:, 1:] == 1.0)
    if not targeted:  # the identity grid gives the clean margin
        one = A.TimeWarp(est, 0.0, counts=(1, 1, 1))
        same = one.generate_device(xt, torch.as_tensor(y), lengths=lengths)
        clean = margin_device(est.predict_device(xt, logits=True, lengths=lengths).contiguous(), torch.as_tensor(y).int().cuda())
        assert torch.equal(one.margins_, clean) and torch.equal(same, xt)
        host = A.TimeWarp(est, 256.0, counts=(9, 1, 1)).generate(x, y, lengths=lengths)  # NumPy in, NumPy out
        assert isinstance(host, np.ndarray) and host.dtype == x.dtype and np.array_equal(host, adv.cpu().numpy())


def test_refinement_lowers_margins_inside_the_box(bed):
    from lipasr import attacks as A

    est, lengths, xt, y = bed["est"], bed["lengths"], bed["xt"], torch.as_tensor(bed["y"])
    coarse = A.TimeWarp(est, 256.0, 1.05, 1.0, counts=(3, 3, 3))
    coarse.generate_device(xt, y, lengths=lengths)
    fine = A.TimeWarp(est, 256.0, 1.05, 1.0, counts=(3, 3, 3), refine_steps=3)
    fine.generate_device(xt, y, lengths=lengths)
    assert bool((fine.margins_ <= coarse.margins_).all()) and bool((fine.margins_ < coarse.margins_).any())
    p = fine.params_.cpu().numpy()
    assert np.all((p >= fine.lo) & (p <= fine.hi))
    print(f"refinement: {int((fine.margins_ < coarse.margins_).sum())} of {len(p)} margins fell")


def test_chunks_give_the_bits_of_one_clip_at_a_time(bed):
    from lipasr import attacks as A

    est = bed["est32"]
    assert est.batch_limit == 32
    reps = np.arange(70) % len(bed["x"])
    xt, lengths, y = bed["xt"][reps].contiguous(), bed["lengths"][reps], torch.as_tensor(bed["y"][reps])
    atk = A.TimeWarp(est, 128.0, counts=(9, 1, 1))  # chunks of 32 // 9 = 3 clips
    adv = atk.generate_device(xt, y, lengths=lengths)
    params, margins = atk.params_.clone(), atk.margins_.clone()
    for b in range(70):
        one = atk.generate_device(xt[b:b + 1], y[b:b + 1], lengths=lengths[b:b + 1])
        assert torch.equal(one[0], adv[b]) and torch.equal(atk.params_[0], params[b]) and torch.equal(atk.margins_[0], margins[b]), b
    with pytest.raises(ValueError):
        A.TimeWarp(est, 128.0, 1.05, 1.0, counts=(9, 3, 3))  # 81 candidates > batch_limit 32


def test_menu_runs_the_time_warp_sweep(cuda, tmp_path, capsys):
    import wave

    import local_lip_ref as L
    from helpers import build_model, load_params
    from lipasr import attack_eval as V
    from lipasr.extract_features_construct_dataset import compute_mfcc_all_files
    from lipasr.synth import synth_clips
    from oracle import mlp_ref as P

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
    lab[-1] = 9
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
    common = ["--path", str(data) + "/", "--noise-dir", str(noise), "--constrained", h5, "--unconstrained", h5, "--kind", "warp"]
    capsys.readouterr()
    # 0, 4, 8, 16 ms with 2^3 + 1 delays each: every grid holds the one before it
    grid, acc = V.main(common + ["--attack", "black", "--over", "audio", "--max-shift-ms", "0", "4", "8", "16"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Accuracy on time-warped audio test examples")]
    assert grid == [0.0, 4.0, 8.0, 16.0] and set(acc) == {"constrained", "unconstrained"} and len(lines) == 8
    for v in acc.values():
        assert len(v) == 4 and np.all((0.0 <= v) & (v <= 1.0)) and np.all(np.diff(v) <= 0)
    grid, acc = V.main(common + ["--attack", "white", "--over", "audio", "--max-shift-ms", "4", "--refine", "1"])
    assert grid == [4.0] and all(len(v) == 1 for v in acc.values())
    for bad in (["--attack", "black", "--over", "mfcc"], ["--attack", "white"], ["--attack", "black", "--over", "audio", "--refine", "2"]):
        with pytest.raises(ValueError):
            V.main(common + bad)
