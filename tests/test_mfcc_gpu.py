"""GPU parity: K1 (resample, STFT, mel, dB, DCT) against oracle.mfcc_ref.

Tolerance: |delta MFCC| <= 2e-2 absolute (coefficients span roughly -700..+200 dB-units; per-feature
standard deviations over a corpus are 5..60, so this is <= 4e-3 standardised units and stays an order
below what a 1e-3 relative logit change needs -- DESIGN.md 'MFCC tolerance').  The resampler alone is
checked to 2e-6, the float32 FFT is the dominant term.
"""
import os

import numpy as np
import pytest
import torch

from golden import inputs
from helpers import dev
from oracle import mfcc_ref as M

pytestmark = pytest.mark.gpu
ATOL = 2e-2


def test_resample_matches_resampy_restatement(cuda):
    from lipasr.extract_features_construct_dataset import MfccExtractor

    clips = inputs.test_clips()
    ex = MfccExtractor(16000, 16000, 8)
    y = ex.resample(dev(clips)).cpu().numpy()
    assert y.shape == (4, 22050)
    for i in range(4):
        np.testing.assert_allclose(y[i], M.librosa_load_resample(clips[i], 16000), atol=2e-6)


def test_mfcc_golden_clips(cuda, golden_dir):
    from lipasr.extract_features_construct_dataset import mfcc

    g = np.load(os.path.join(golden_dir, "mfcc.npz"))
    got = mfcc(inputs.test_clips()).cpu().numpy()
    assert got.shape == (4, 880)
    assert np.abs(got - g["feats"]).max() < ATOL
    assert np.abs(got - M.compute_mfcc_batch(inputs.test_clips())).max() < ATOL


def test_mfcc_synthetic_batch_and_layout(cuda):
    from lipasr.extract_features_construct_dataset import mfcc
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(24, seed=77)
    got = mfcc(waves).cpu().numpy()
    ref = M.compute_mfcc_batch(waves)
    assert np.abs(got - ref).max() < ATOL
    # coefficient-major: feature index = coeff*44 + frame (extract_features_construct_dataset.py:145-149)
    one = M.extract_features_wave(waves[3])
    assert np.abs(got[3].reshape(20, 44) - one).max() < ATOL


def test_mfcc_edge_cases(cuda, golden_dir):
    from lipasr.extract_features_construct_dataset import mfcc

    g = np.load(os.path.join(golden_dir, "mfcc.npz"))
    clips = inputs.test_clips()
    # all-zero clip: amin floor and top_db leave -100 dB everywhere -> c0 = -100*sqrt(128), rest 0
    z = mfcc(np.zeros((2, 16000), np.float32)).cpu().numpy().reshape(2, 20, 44)
    np.testing.assert_allclose(z[:, 0], -100.0 * np.sqrt(128.0), rtol=1e-5)
    assert np.abs(z[:, 1:]).max() < 1e-3
    # shorter than 1 s: 21 frames, then literal zeros (extract_features...py:33-37); 7430*22050/16000 is not an integer
    short = mfcc(clips[:2, :7430]).cpu().numpy()
    assert np.abs(short - g["short"]).max() < ATOL
    assert np.all(short.reshape(2, 20, 44)[:, :, 21:] == 0.0)
    # longer than 1 s: 65 frames, truncated at 44, but top_db uses the max over all 65
    long = np.concatenate([clips[:2], clips[:2, :8000]], axis=1)
    got = mfcc(long).cpu().numpy()
    assert np.abs(got - g["long"]).max() < ATOL
    # other utterance lengths
    got30 = mfcc(clips[:2], utterance_length=30).cpu().numpy().reshape(2, 20, 30)
    full = g["feats"][:2].reshape(2, 20, 44)
    assert np.abs(got30 - full[:, :, :30]).max() < ATOL


@pytest.mark.parametrize("sr_in", [22050, 8000, 44100])
def test_other_sample_rates(cuda, sr_in):
    from lipasr.extract_features_construct_dataset import mfcc

    rng = np.random.default_rng(sr_in)
    n = sr_in // 2
    t = np.arange(n) / sr_in
    w = (0.3 * np.sin(2 * np.pi * 700 * t) + 0.02 * rng.standard_normal(n)).astype(np.float32)[None, :]
    got = mfcc(w, sr_in=sr_in).cpu().numpy()
    ref = M.compute_mfcc_batch(w, sr_in=sr_in)
    assert np.abs(got - ref).max() < ATOL  # 44100 -> 22050 has an exact time register (step 2.0), so no phase-0 quirk


def test_fused_standardisation_and_scaler(cuda):
    from lipasr.attacks import StandardScaler, standardize_dataset
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips
    from oracle import mlp_ref as P

    waves, _ = synth_clips(48, seed=5)
    ex = MfccExtractor(16000, 16000, 64)
    feats = ex(dev(waves))
    sc = StandardScaler().fit(feats)
    mean_ref, scale_ref = P.standard_scaler_fit(feats.cpu().numpy().astype(np.float64))
    np.testing.assert_allclose(sc.mean_.cpu().numpy(), mean_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sc.scale_.cpu().numpy(), scale_ref, rtol=1e-12)
    fused = ex(dev(waves), 44, sc.mean_, sc.scale_).cpu().numpy()
    ref = (feats.cpu().numpy().astype(np.float64) - mean_ref) / scale_ref
    np.testing.assert_allclose(fused, ref, atol=1e-5)
    a, b, c = standardize_dataset(feats[:20].cpu().numpy(), feats[20:30].cpu().numpy(), feats[30:].cpu().numpy())
    np.testing.assert_allclose(np.concatenate([a, b, c]), ref, atol=1e-5)
    const = np.ones((10, 3), np.float32) * np.array([1.0, 0.0, 5.0], np.float32)
    s2 = StandardScaler().fit(const)
    assert np.all(s2.scale_.cpu().numpy() == 1.0)


def test_mfcc_needs_plan_and_validates(cuda):
    from lipasr import _native as N
    import ctypes as C

    h = N.c_h()
    N.check(N.lib.lipasr_create(0, C.byref(h)))
    out = torch.zeros(1, 880, device="cuda")
    w = torch.zeros(1, 16000, device="cuda")
    assert N.lib.lipasr_mfcc_f32(h, N.ptr(w), 1, 44, None, None, N.ptr(out), N.stream_ptr()) == N.ESTATE
    assert "lipasr_mfcc_plan" in N.last_error()
    assert N.lib.lipasr_mfcc_plan(h, 16000, 1, 1) == N.EINVAL
    N.check(N.lib.lipasr_mfcc_plan(h, 16000, 16000, 2))
    assert N.lib.lipasr_mfcc_f32(h, N.ptr(w), 3, 44, None, None, N.ptr(out), N.stream_ptr()) == N.EINVAL  # batch > plan
    N.check(N.lib.lipasr_destroy(h))


# ------------------------------------------------------------------ round 3: fused resample -> STFT kernel, int16 PCM, ragged batches
def test_fused_kernel_equals_three_kernel_path(cuda):
    """mfcc_fused_kernel (resampled signal in LDS, 16x16x4 MFMA rows = q-blocks of one clip) against the round-2 path
    (resample_persist -> HBM -> stft_mel), same plan, stage-mask bit 7.  Both resamplers run the same ascending-k fp32 fma
    chain, so the difference is the FFT twiddles (table values vs products of table values): ~1e-5 in MFCC units."""
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(40, seed=11)
    ex = MfccExtractor(16000, 16000, 64)
    assert ex.fused  # the plan CAN fuse; by default it does so only for int16 / ragged input
    b = ex(dev(waves)).cpu().numpy()  # default: three-kernel path, dual-FFT STFT kernel
    ex.set(0, 64)  # ... with the round-2 one-pair-per-workgroup STFT kernel
    b2 = ex(dev(waves)).cpu().numpy()
    ex.set(0, 0)
    ex.set(2, 1)  # the fused kernel for every batch
    a = ex(dev(waves)).cpu().numpy()
    c = ex(dev(waves)).cpu().numpy()
    assert np.array_equal(a, c)  # deterministic
    assert np.abs(a - b).max() < 2e-3, np.abs(a - b).max()
    assert np.abs(b - b2).max() < 2e-3, np.abs(b - b2).max()  # dual-FFT kernel (four frames per workgroup) vs the pair kernel
    ref = M.compute_mfcc_batch(waves[:8])
    assert max(np.abs(x[:8] - ref).max() for x in (a, b, b2)) < ATOL


@pytest.mark.parametrize("n", [22050, 9000, 1500, 23000, 2])
def test_dual_fft_kernel_frame_counts(cuda, n):
    """stft_mel2_kernel handles four frames per workgroup: frame counts 44 (multiple of 4), 18 and 45 (partial last quad,
    incl. a lone fifth frame), 3 (every frame reflects) and 1, on 22 050 Hz input (no resampler in the way)."""
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(n)
    w = (0.2 * rng.standard_normal((3, n))).astype(np.float32)
    ex = MfccExtractor(22050, n, 4)
    L = 1 + n // 512
    got = ex(dev(w), L).cpu().numpy()
    ref = M.compute_mfcc_batch(w, sr_in=22050, utterance_length=L)
    assert np.abs(got - ref).max() < ATOL, np.abs(got - ref).max()
    ex.set(0, 64)
    old = ex(dev(w), L).cpu().numpy()
    assert np.abs(got - old).max() < 2e-3


@pytest.mark.parametrize("sr_in,n", [(16000, 16000), (8000, 8000), (16000, 24000), (16000, 5003)])
def test_fused_kernel_other_rates_and_lengths(cuda, sr_in, n):
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(n)
    t = np.arange(n) / sr_in
    w = (0.3 * np.sin(2 * np.pi * (300 + 200 * np.arange(5)[:, None]) * t) + 0.05 * rng.standard_normal((5, n))).astype(np.float32)
    ex = MfccExtractor(sr_in, n, 8)
    assert ex.fused
    ex.set(2, 1)
    got = ex(dev(w), 50).cpu().numpy()
    ref = M.compute_mfcc_batch(w, sr_in=sr_in, utterance_length=50)
    assert np.abs(got - ref).max() < ATOL, np.abs(got - ref).max()


def test_int16_pcm_input_is_bit_identical(cuda):
    """lipasr_mfcc_i16 / sample_format 1: the device scales by 2^-15 while staging, which is exactly the host conversion
    (extract_features_construct_dataset.py:27, librosa.load's decode of 16-bit PCM).  Both forms of the path: the three
    kernels (the resampler reads int16 directly) and the fused resample+STFT kernel."""
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(19, seed=3)
    pcm = np.clip(np.round(waves * 32768.0), -32768, 32767).astype(np.int16)
    ref = M.compute_mfcc_batch(pcm.astype(np.float32) / 32768.0)
    ex = MfccExtractor(16000, 16000, 32)
    res = {}
    for fused in (0, 1):
        ex.set(2, fused)
        a = ex(torch.as_tensor(pcm).cuda())
        b = ex(dev(pcm.astype(np.float32) / 32768.0))
        assert torch.equal(a, b), fused
        assert np.abs(a.cpu().numpy() - ref).max() < ATOL
        res[fused] = a
    assert (res[0] - res[1]).abs().max() < 1e-3  # two kernels, one algorithm (fp16-plane vs fp32 resampling, other twiddles)
    # a row length that is not a multiple of 4 (no vector loads: the plan falls back to the fused kernel by itself) and the
    # handle-level C entry point
    import ctypes as C

    from lipasr import _native as N

    odd = pcm[:, :15999].copy()
    exo = MfccExtractor(16000, 15999, 32)
    oi, of = exo(torch.as_tensor(odd).cuda()), exo(dev(odd.astype(np.float32) / 32768.0))  # fused kernel | fp32 three-kernel path
    assert (oi - of).abs().max() < 1e-3
    exo.set(2, 1)
    assert torch.equal(oi, exo(dev(odd.astype(np.float32) / 32768.0)))
    h = N.get_handle(0)
    N.check(N.lib.lipasr_mfcc_plan(h.h, 16000, 16000, 32))
    out = torch.empty(19, 880, device="cuda")
    N.check(N.lib.lipasr_mfcc_i16(h.h, N.ptr(torch.as_tensor(pcm).cuda()), None, 19, 44, None, None, N.ptr(out), N.stream_ptr()))
    assert torch.equal(out, res[0])


@pytest.mark.parametrize("fused", [0, 1])
def test_ragged_batch_equals_per_clip_launches(cuda, fused):
    """Clips of different lengths in ONE launch (compute_mfcc_all_files loops files of any length,
    extract_features_construct_dataset.py:144-150): clip u with n_valid[u] samples comes out exactly as a plan made
    for that length produces it alone -- resampled length, frame count, reflect padding, the top_db maximum and the zero
    columns past its last frame.  Garbage beyond n_valid in a row must not matter.  fused = 0: the three kernels
    (resample_persist_h2_kernel<., true> cuts each row at its clip's end, stft_mel2_kernel takes per-clip lengths);
    fused = 1: mfcc_fused_kernel."""
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(12, seed=9)
    lens = np.array([16000, 15999, 12345, 8000, 7430, 4096, 2049, 1025, 700, 37, 2, 16000], dtype=np.int32)
    rng = np.random.default_rng(0)
    padded = waves.copy()
    for i, n in enumerate(lens):
        padded[i, n:] = rng.standard_normal(16000 - n)  # not zeros: the tail is outside the clip
    ex = MfccExtractor(16000, 16000, 16)
    ex.set(2, fused)
    sc_mean = torch.as_tensor(rng.standard_normal(880)).cuda()
    sc_scale = torch.as_tensor(rng.uniform(0.5, 2.0, 880)).cuda()
    got = ex(dev(padded), n_valid=torch.as_tensor(lens).cuda())
    got_aff = ex(dev(padded), 44, sc_mean, sc_scale, n_valid=torch.as_tensor(lens).cuda())
    for i, n in enumerate(lens):
        one = MfccExtractor(16000, int(n), 1)
        one.set(2, fused)
        alone = one(dev(waves[i:i + 1, :n]))
        alone_aff = one(dev(waves[i:i + 1, :n]), 44, sc_mean, sc_scale)
        # the same kernels as the ragged launch -> bit-identical.  (Three-kernel form: a row length that is not a multiple of 4
        # sends the single-clip plan to another resampling kernel, fp32 instead of fp16 planes: same algorithm, ~1e-5 apart.)
        if fused or n % 4 == 0:
            assert torch.equal(got[i:i + 1], alone), (i, n, float((got[i:i + 1] - alone).abs().max()))
            assert torch.equal(got_aff[i:i + 1], alone_aff), (i, n)
        else:
            assert (got[i:i + 1] - alone).abs().max() < 1e-3, (i, n, float((got[i:i + 1] - alone).abs().max()))
            assert (got_aff[i:i + 1] - alone_aff).abs().max() < 2e-3, (i, n)
        ref = M.compute_mfcc_batch(waves[i:i + 1, :n])
        assert np.abs(got[i:i + 1].cpu().numpy() - ref).max() < ATOL, (i, n)
        one.close()
    # int16 + ragged together, and through the module-level entry (the default form of the path)
    from lipasr.extract_features_construct_dataset import mfcc

    pcm = np.clip(np.round(padded * 32768.0), -32768, 32767).astype(np.int16)
    a = mfcc(pcm, 16000, n_valid=lens)
    b = mfcc(pcm.astype(np.float32) / 32768.0, 16000, n_valid=lens)
    assert torch.equal(a, b)
    # the ragged launch with every clip full-length is the plain launch
    full = torch.full((12,), 16000, dtype=torch.int32, device="cuda")
    assert torch.equal(ex(dev(waves), n_valid=full), ex(dev(waves)))
    # a zero-length row has no frame at all -> the zero columns of fix_frames; one sample resamples to ceil(1.378) = 2
    # samples = one frame, zero columns after it
    z = ex(dev(padded[:2]), n_valid=torch.as_tensor(np.array([0, 1], np.int32)).cuda()).cpu().numpy().reshape(2, 20, 44)
    assert np.count_nonzero(z[0]) == 0
    assert np.isfinite(z[1]).all() and np.count_nonzero(z[1, :, 1:]) == 0 and z[1, 0, 0] < -100.0
    ex.close()


def test_ragged_batch_large_and_mixed(cuda):
    """A loader-sized ragged int16 batch (random lengths, 300 clips: several 32-row tiles, tiles whose last rows are missing)
    through the three-kernel form against the fused kernel; both cut every clip at its own end."""
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(300, seed=21)
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 16001, size=300).astype(np.int32)
    lens[:7] = [16000, 15997, 15998, 15999, 3, 4, 5]
    pcm = np.clip(np.round(waves * 32768.0), -32768, 32767).astype(np.int16)
    for i, n in enumerate(lens):
        pcm[i, n:] = rng.integers(-30000, 30000, size=16000 - n)
    ex = MfccExtractor(16000, 16000, 300)
    nv = torch.as_tensor(lens).cuda()
    a = ex(torch.as_tensor(pcm).cuda(), n_valid=nv)
    ex.set(2, 1)
    b = ex(torch.as_tensor(pcm).cuda(), n_valid=nv)
    d = (a - b).abs().amax(dim=1).cpu().numpy()
    assert d.max() < 1e-3, (int(d.argmax()), int(lens[d.argmax()]), float(d.max()))
    # and a sample of rows against the oracle
    for i in (0, 1, 2, 3, 4, 5, 6, 50, 131, 299):
        ref = M.compute_mfcc_batch(pcm[i:i + 1, :lens[i]].astype(np.float32) / 32768.0)
        assert np.abs(a[i:i + 1].cpu().numpy() - ref).max() < ATOL, (i, int(lens[i]))
    ex.close()


def test_ragged_and_int16_unsupported_plans_say_so(cuda):
    from lipasr.extract_features_construct_dataset import MfccExtractor

    ex = MfccExtractor(44100, 4410, 4)  # a down-sampling rate: no fp16-plane resampler, no fused kernel
    assert not ex.fused
    w = torch.zeros(2, 4410, device="cuda")
    ex(w)
    import lipasr._native as N

    with pytest.raises(N.LipasrError) as e:
        ex(w, n_valid=torch.full((2,), 4000, dtype=torch.int32, device="cuda"))
    assert e.value.code == N.EUNSUPPORTED
    with pytest.raises(N.LipasrError) as e:
        ex(torch.zeros(2, 4410, dtype=torch.int16, device="cuda"))
    assert e.value.code == N.EUNSUPPORTED


def test_two_extractors_do_not_share_state(cuda):
    """one MFCC plan per handle made alternating extractors re-plan on every call; plans are objects now."""
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(8, seed=1)
    a, b = MfccExtractor(16000, 16000, 8), MfccExtractor(16000, 8000, 8)
    fa = a(dev(waves))
    fb = b(dev(waves[:, :8000].copy()))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        fa2 = a(dev(waves))
    with torch.cuda.stream(s2):
        fb2 = b(dev(waves[:, :8000].copy()))
    torch.cuda.synchronize()
    assert torch.equal(fa, fa2) and torch.equal(fb, fb2)
    a.close(); b.close()
    with pytest.raises(Exception):
        a(dev(waves))


def test_fp16_plane_resampler_against_fp32_kernel_and_oracle(cuda):
    """resample_persist_h2_kernel (two fp16 planes per operand on v_mfma_f32_32x32x16_f16, three cross terms) against the exact
    fp32 MFMA kernel (stage-mask bit 4, the parity reference) and the float64 oracle, on full-scale white noise -- the worst
    case for the dropped 2^-22 terms -- and on quiet speech-like clips; 16 kHz and 8 kHz input."""
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    rng = np.random.default_rng(5)
    loud = rng.uniform(-1.0, 1.0, (6, 16000)).astype(np.float32)
    quiet, _ = synth_clips(6, seed=8)
    quiet = (1e-3 * quiet).astype(np.float32)
    for sr, clips in ((16000, np.concatenate([loud, quiet])), (8000, np.concatenate([loud[:, :8000], quiet[:, :8000]]))):
        ex = MfccExtractor(sr, clips.shape[1], 40)
        y_h2 = ex.resample(dev(clips)).cpu().numpy()
        ex.set(0, 16)
        y_f32 = ex.resample(dev(clips)).cpu().numpy()
        ex.set(0, 0)
        ref = np.stack([M.librosa_load_resample(c, sr) for c in clips])
        e_h2, e_f32 = np.abs(y_h2 - ref).max(axis=1), np.abs(y_f32 - ref).max(axis=1)
        print(f"\nresampler {sr} Hz: max|err| vs float64 oracle  fp16-plane {e_h2[:6].max():.2e} (loud) {e_h2[6:].max():.2e} (quiet)   "
              f"fp32 {e_f32[:6].max():.2e} / {e_f32[6:].max():.2e}")
        assert e_f32.max() < 2e-6 and e_h2.max() < 2e-6
        assert e_h2[6:].max() < 2e-9          # relative, not absolute: a clip at -60 dB is as accurate as a loud one
        assert np.abs(y_h2 - y_f32).max() < 2e-6


def test_mfma_and_reg128_resamplers_against_oracle(cuda):
    """The two 16 kHz resampler variants no other test reaches, on full-scale uniform noise against the float64 oracle, to the
    2e-6 absolute error the other fp32 resamplers are held to: resample_mfma_kernel (the default choice for rows that cannot be
    read as float4: 1602 samples) and resample_reg128_kernel (stage-mask bit 2 = 4, rows of 1600)."""
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(11)
    for n, mask, name in ((1602, 0, "resample_mfma_kernel"), (1600, 4, "resample_reg128_kernel")):
        clips = rng.uniform(-1.0, 1.0, (3, n)).astype(np.float32)
        ex = MfccExtractor(16000, n, 3)
        ex.set(0, mask)
        y = ex.resample(dev(clips)).cpu().numpy()
        ex.close()
        ref = np.stack([M.librosa_load_resample(c, 16000) for c in clips])
        err = np.abs(y - ref).max()
        print(f"\n{name}: rows of {n}, max|err| vs float64 oracle {err:.2e}")
        assert y.shape == ref.shape and err < 2e-6, (name, err)


# ------------------------------------------------------------------ round 4: block-DFT STFT kernel on the matrix pipe
def test_block_dft_kernel_against_stockham_kernel_and_oracle(cuda):
    """stft_bdft_kernel (default since round 4: block spectra on v_mfma_f32_32x32x16_f16 with two fp16 planes, Hann as three
    frequency-domain taps) against stft_mel2_kernel (stage-mask bit 8, the fp32 Stockham FFT: the parity reference) and the
    float64 oracle, on clips that stress the scheme: full-scale white noise (largest rounding), a pure tone (the Hann taps
    cancel three large rectangular-window bins into a small one far from the peak), a tone over a -90 dB floor, a quiet
    clip (fp16 planes near their subnormal range) and a chirp.  VERDICT r3 item 2: new within 2e-3 of old, both within ATOL."""
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(4)
    n = 22050
    t = np.arange(n) / 22050.0
    w = np.stack([
        rng.uniform(-1, 1, n),
        0.5 * np.sin(2 * np.pi * 1000.3 * t),
        0.5 * np.sin(2 * np.pi * 5000.7 * t) + 1.5e-5 * rng.standard_normal(n),
        1e-4 * rng.standard_normal(n),
        0.3 * np.sin(2 * np.pi * (200 * t + 4000 * t * t)),
        0.2 * rng.standard_normal(n) * (t > 0.5),
    ]).astype(np.float32)
    ex = MfccExtractor(22050, n, 8)
    new = ex(dev(w), 44).cpu().numpy()
    again = ex(dev(w), 44).cpu().numpy()
    assert np.array_equal(new, again)  # deterministic
    ex.set(0, 256)
    old = ex(dev(w), 44).cpu().numpy()
    ex.set(0, 0)
    ref = M.compute_mfcc_batch(w, sr_in=22050, utterance_length=44)
    d_new, d_old, d_no = np.abs(new - ref).max(axis=1), np.abs(old - ref).max(axis=1), np.abs(new - old).max(axis=1)
    print("\nblock-DFT vs oracle", d_new, "\nStockham vs oracle ", d_old, "\nblock-DFT vs Stockham", d_no)
    assert d_no.max() < 2e-3, d_no
    assert d_new.max() < ATOL and d_old.max() < ATOL


@pytest.mark.parametrize("L", [44, 30, 50, 64])
def test_fused_dct_epilogue_is_bit_identical_to_dct_kernel(cuda, L):
    """One workgroup per clip, on request (plan key 4): stft_bdft_kernel ends with the top_db floor and the DCT itself (no
    dct_kernel launch, the dB tile comes back from L2).  Same instructions in the same order as dct_kernel => the same bits, with and without the fused
    StandardScaler affine, for utterance lengths shorter and longer than the clip's 44 frames; ragged batches too."""
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(37, seed=5)
    ex = MfccExtractor(16000, 16000, 64)
    wt = dev(waves)
    mean = torch.linspace(-3, 3, 20 * L, device="cuda", dtype=torch.float64)
    scale = torch.linspace(0.5, 2, 20 * L, device="cuda", dtype=torch.float64)
    nv = torch.as_tensor(np.random.default_rng(L).integers(1000, 16001, 37).astype(np.int32) // 4 * 4).cuda()
    outs = {}
    for fuse in (0, 1):  # plan key 4: the STFT kernel's own DCT epilogue
        ex.set(4, fuse)
        outs[fuse] = (ex(wt, L).clone(), ex(wt, L, mean, scale).clone(), ex(wt, L, n_valid=nv).clone())
    ex.set(4, 0)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
