"""extract_features_construct_dataset.py surface (reference :24-39, :144-196) over liblipasr.

* ``extract_features(file_path, utterance_length)`` / ``compute_mfcc_all_files(filenames)`` keep the
  reference signatures; the wav is decoded on the host (stdlib ``wave``: 16-bit PCM, what the Speech
  Commands corpus ships) and everything after decoding -- resampling to 22 050 Hz, STFT, mel, dB,
  DCT, pad/trim, flatten -- runs in the K1 kernels, batched.
* ``mfcc(waveforms, sr_in)`` is the batched tensor entry the GPU pipeline uses.
* ``get_norms`` / ``get_upper_lipschitz`` / ``get_lipschitz_constrained`` are the Lipschitz
  read-outs, computed by the K3 kernels instead of host SVDs.
* ``get_lipschitz_bound`` / ``get_robustness_radius`` (ours) put a certified radius next to the distance DeepFool finds.
* ``jacobian_sigma`` / ``get_local_lipschitz`` (ours: the reference has no such read-out) measure how much of those
  bounds a model uses at given inputs: the spectral norm of its Jacobian per row.
"""
from __future__ import annotations

import ctypes as C
import wave

import numpy as np
import torch

from . import _native as N
from . import estimators as E  # the module, not its names: it imports this one for the extractor
from .keras import Model

STANDARD_UTTERANCE_LENGTH = 44  # reference :18
N_MFCC = 20


class MfccExtractor:
    """One native MFCC plan (lipasr_mfcc_create: tables + intermediates of its own) for clips of up to ``n_samp`` samples
    at ``sr_in`` Hz, ``batch_max`` clips per launch.  Extractors do not share state: a pipeline's and a validation
    pass's extractor, or two streams, coexist on one handle.  ``n_fft`` / ``hop`` other than 2048 / 512 select the
    short-window path (Speaker recognition)."""

    def __init__(self, sr_in=16000, n_samp=16000, batch_max=512, device=None, n_fft=2048, hop=512):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.h = N.get_handle(self.device.index)
        self.sr_in, self.n_samp, self.batch_max = int(sr_in), int(n_samp), int(batch_max)
        self.n_fft, self.hop = int(n_fft), int(hop)
        self.short_window = (self.n_fft, self.hop) != (2048, 512)  # the plan runs the DFT-contraction path
        plan = N.c_h()
        N.check(N.lib.lipasr_mfcc_create(self.h.h, self.sr_in, self.n_samp, self.batch_max, int(n_fft), int(hop), C.byref(plan)))
        self._plan = plan
        N.register_owner(self)
        ny, nf, fu = C.c_int(), C.c_int(), C.c_int()
        N.check(N.lib.lipasr_mfcc_plan_dims(plan, C.byref(ny), C.byref(nf), C.byref(fu)))
        self.n_y, self.n_frames, self.fused = ny.value, nf.value, bool(fu.value)

    def close(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan and self.h.alive:
            N.destroy_or_defer(N.lib.lipasr_mfcc_destroy, plan)  # (a finaliser may run in the middle of a graph capture)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, key, value):
        """lipasr_mfcc_plan_set: key 0 = stage mask (every bit is listed at lipasr_mfcc_plan_set in include/lipasr.h), key 1 =
        resampler workgroups, key 2 = 1: the fused resample -> STFT kernel for every batch (default: only where the three
        kernels cannot read the input: int16 / ragged rows that are not a multiple of 4 samples long), key 3 = frames per
        workgroup of the block-DFT kernel (a multiple of 4, default 44); key 4 = 1: that kernel also applies the top_db floor
        and the DCT (no dct_kernel launch; bit-identical, slower on cache-cold batches)."""
        N.check(N.lib.lipasr_mfcc_plan_set(self._plan, int(key), int(value)))

    def profile_begin(self, max_calls):
        N.check(N.lib.lipasr_mfcc_plan_profile_begin(self._plan, int(max_calls)))

    def profile_end(self):
        """-> ({'resample', 'stft_mel', 'dct'} mean milliseconds, number of extractions timed)"""
        ms3, n = (C.c_float * 3)(), C.c_int()
        N.check(N.lib.lipasr_mfcc_plan_profile_end(self._plan, ms3, C.byref(n)))
        return {"resample": ms3[0], "stft_mel": ms3[1], "dct": ms3[2]}, n.value

    def __call__(self, waves, utterance_length=STANDARD_UTTERANCE_LENGTH, mean=None, scale=None, out=None, n_valid=None):
        """waves: device tensor [B, n_samp], float32 in [-1, 1) or int16 PCM -> [B, 20*utterance_length] (coefficient-major).
        n_valid: int32 device tensor [B]: samples of each row that belong to the clip (clips of different lengths in one
        launch; the rest of a row is ignored)."""
        if self._plan is None:
            raise RuntimeError("MfccExtractor used after close()")
        b = waves.shape[0]
        if waves.shape[1] != self.n_samp or not waves.is_contiguous():
            raise ValueError(f"waves must be contiguous [B, {self.n_samp}], got {tuple(waves.shape)}")
        if waves.dtype == torch.int16:
            fmt = 1
        elif waves.dtype == torch.float32:
            fmt = 0
        else:
            raise ValueError(f"waves must be float32 or int16, got {waves.dtype}")
        if n_valid is not None and (n_valid.dtype != torch.int32 or n_valid.shape[0] != b):
            raise ValueError("n_valid must be an int32 device tensor [B]")
        if out is None:
            out = torch.empty(b, N_MFCC * utterance_length, device=self.device)
        N.check(N.lib.lipasr_mfcc_extract(self._plan, N.ptr(waves), fmt, N.ptr(n_valid), b, utterance_length, N.ptr(mean), N.ptr(scale),
                                          N.ptr(out), N.stream_ptr()))
        return out

    def _lengths(self, n_valid, b):
        if not torch.is_tensor(n_valid) or n_valid.dtype != torch.int32 or tuple(n_valid.shape) != (b,) or not n_valid.is_cuda \
                or not n_valid.is_contiguous():
            raise ValueError(f"n_valid must be a contiguous int32 device tensor [{b}]")
        return n_valid

    def resample(self, waves, out=None, n_valid=None):
        """[B, n_samp] at sr_in -> [B, n_y] at 22 050 Hz.  n_valid (int32 device tensor [B], samples at sr_in): clips of different
        lengths (lipasr_mfcc_plan_resample_ragged; float32 or int16 rows); every row is zero from int(n * 22050 / sr_in) on."""
        y = torch.empty(waves.shape[0], self.n_y, device=self.device) if out is None else out
        if n_valid is None:
            N.check(N.lib.lipasr_mfcc_plan_resample(self._plan, N.ptr(waves), waves.shape[0], N.ptr(y), N.stream_ptr()))
            return y
        b = waves.shape[0]
        if waves.dim() != 2 or waves.shape[1] != self.n_samp or not waves.is_contiguous() or waves.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"waves must be contiguous float32 or int16 [B, {self.n_samp}], got {waves.dtype} {tuple(waves.shape)}")
        if tuple(y.shape) != (b, self.n_y) or y.dtype != torch.float32 or not y.is_contiguous():
            raise ValueError(f"out must be contiguous float32 [{b}, {self.n_y}]")
        N.check(N.lib.lipasr_mfcc_plan_resample_ragged(self._plan, N.ptr(waves), 1 if waves.dtype == torch.int16 else 0,
                                                       N.ptr(self._lengths(n_valid, b)), b, N.ptr(y), N.stream_ptr()))
        return y

    def from_22k(self, y, utterance_length=STANDARD_UTTERANCE_LENGTH, mean=None, scale=None, out=None, n_valid=None):
        """[B, n_y] at 22 050 Hz -> features.  n_valid (int32 device tensor [B]): clips of different lengths, counted in samples at
        sr_in as everywhere else; a row holds its clip in its first ceil(n * 22050 / sr_in) positions
        (lipasr_mfcc_plan_from_22k_ragged)."""
        if out is None:
            out = torch.empty(y.shape[0], N_MFCC * utterance_length, device=self.device)
        if n_valid is None:
            N.check(N.lib.lipasr_mfcc_plan_from_22k(self._plan, N.ptr(y), y.shape[0], y.shape[1], utterance_length, N.ptr(mean), N.ptr(scale),
                                                    N.ptr(out), N.stream_ptr()))
            return out
        b = y.shape[0]
        if y.dim() != 2 or y.shape[1] != self.n_y or y.dtype != torch.float32 or not y.is_contiguous():
            raise ValueError(f"y must be contiguous float32 [B, {self.n_y}], got {y.dtype} {tuple(y.shape)}")
        if tuple(out.shape) != (b, N_MFCC * utterance_length) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be contiguous float32 [{b}, {N_MFCC * utterance_length}]")
        N.check(N.lib.lipasr_mfcc_plan_from_22k_ragged(self._plan, N.ptr(y), N.ptr(self._lengths(n_valid, b)), b, int(utterance_length),
                                                       N.ptr(mean), N.ptr(scale), N.ptr(out), N.stream_ptr()))
        return out

    def _vjp_args(self, sig, g_feat, utterance_length, scale, domain, out, dtypes):
        """The argument check of ``vjp`` / ``vjp_short`` / ``vjp_ragged`` -> (domain code, B, the gradient buffer).  dtypes: what
        ``sig`` may be (``vjp`` lets int16 through so that the caller sees the library's EUNSUPPORTED)."""
        if self._plan is None:
            raise RuntimeError("MfccExtractor used after close()")
        if domain not in ("input", "22k"):
            raise ValueError(f"domain={domain!r}: 'input' or '22k'")
        dom = 0 if domain == "input" else 1
        n = self.n_samp if dom == 0 else self.n_y
        b = sig.shape[0]
        if sig.dim() != 2 or sig.shape[1] != n or not sig.is_contiguous():
            raise ValueError(f"sig must be contiguous [B, {n}] for domain {domain!r}, got {tuple(sig.shape)}")
        if sig.dtype not in dtypes:
            raise ValueError(f"sig must be {' or '.join(str(d).split('.')[-1] for d in dtypes)}, got {sig.dtype}")
        if tuple(g_feat.shape) != (b, N_MFCC * utterance_length) or g_feat.dtype != torch.float32 or not g_feat.is_contiguous():
            raise ValueError(f"g_feat must be contiguous float32 [{b}, {N_MFCC * utterance_length}]")
        if scale is not None and (scale.dtype != torch.float64 or scale.numel() != N_MFCC * utterance_length):
            raise ValueError("scale must be a float64 device tensor [20 * utterance_length]")
        if out is None:
            out = torch.empty(b, n, device=self.device)
        elif tuple(out.shape) != (b, n) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be contiguous float32 [{b}, {n}]")
        return dom, b, out

    def vjp(self, sig, g_feat, utterance_length=STANDARD_UTTERANCE_LENGTH, scale=None, domain="input", reuse_forward=False, out=None,
            n_valid=None):
        """Backward pass (lipasr_mfcc_plan_vjp): the gradient w.r.t. ``sig`` of <features(sig), g_feat>.
        domain="input": sig [B, n_samp] at sr_in (what ``__call__`` takes); domain="22k": sig [B, n_y] (what ``from_22k`` takes).
        scale: the float64 StandardScaler scale the forward applied, or None.  reuse_forward=True: this extractor's last call
        was the forward on exactly this ``sig`` on the current stream; the resampled signal it left is read, and its dB tile too
        where stft_mel2_kernel made it (stage-mask bit 256; otherwise that kernel runs again for the backward pass: the default
        block-DFT tile is not accurate enough to divide by).  The bits are the same either way.
        2048/512 plans, float32 rows of one length: anything else raises LipasrError(EUNSUPPORTED).  Clips of different lengths
        in one launch, int16 rows and clips shorter than the reflect padding: ``vjp_ragged``; short-window extractors: ``vjp_short``."""
        dom, b, out = self._vjp_args(sig, g_feat, utterance_length, scale, domain, out, (torch.float32, torch.int16))
        flags = (1 if reuse_forward else 0) | (2 if sig.dtype == torch.int16 else 0) | (4 if n_valid is not None else 0)
        N.check(N.lib.lipasr_mfcc_plan_vjp(self._plan, N.ptr(sig), dom, b, int(utterance_length), N.ptr(scale), N.ptr(g_feat), N.ptr(out),
                                           flags, N.stream_ptr()))
        return out

    def vjp_short(self, sig, g_feat, utterance_length, scale=None, domain="22k", reuse_forward=False, out=None):
        """``vjp`` for a short-window extractor (n_fft / hop other than 2048 / 512; lipasr_mfcc_plan_vjp_short): the gradient w.r.t.
        ``sig`` of <features(sig), g_feat>, float32 rows of one length.  domain="22k": sig [B, n_y] (what ``from_22k`` takes);
        domain="input": sig [B, n_samp] at sr_in.  scale and reuse_forward as in ``vjp``.  A 2048/512 extractor raises
        LipasrError(EUNSUPPORTED): ``vjp`` is for those."""
        dom, b, out = self._vjp_args(sig, g_feat, utterance_length, scale, domain, out, (torch.float32,))
        N.check(N.lib.lipasr_mfcc_plan_vjp_short(self._plan, N.ptr(sig), dom, b, int(utterance_length), N.ptr(scale), N.ptr(g_feat),
                                                 N.ptr(out), 1 if reuse_forward else 0, N.stream_ptr()))
        return out

    def vjp_ragged(self, sig, g_feat, n_valid, utterance_length=STANDARD_UTTERANCE_LENGTH, scale=None, domain="input", reuse_forward=False,
                   out=None):
        """``vjp`` for clips of different lengths in one launch (lipasr_mfcc_plan_vjp_ragged).  n_valid: int32 device tensor [B],
        the samples of each row that belong to its clip, counted at sr_in for BOTH domains; a domain="22k" row holds its clip in
        its first ceil(n * 22050 / sr_in) positions.  sig: float32, or int16 PCM for domain="input" (the gradient is float32, with
        respect to pcm / 32768).  The gradient is exactly 0 from each clip's end to the end of its row; a clip may be as short as
        2 resampled samples, and an empty one gets zeros.  reuse_forward=True: this extractor's last call on the current stream was
        the forward with the same rows and n_valid (``__call__`` / ``from_22k`` with n_valid); what is reused: as in ``vjp``.  16 kHz and 8 kHz 2048/512 plans with
        rows a multiple of 4 samples: anything else raises LipasrError(EUNSUPPORTED)."""
        dom, b, out = self._vjp_args(sig, g_feat, utterance_length, scale, domain, out, (torch.float32, torch.int16))
        N.check(N.lib.lipasr_mfcc_plan_vjp_ragged(self._plan, N.ptr(sig), 1 if sig.dtype == torch.int16 else 0, N.ptr(self._lengths(n_valid, b)),
                                                  dom, b, int(utterance_length), N.ptr(scale), N.ptr(g_feat), N.ptr(out),
                                                  1 if reuse_forward else 0, N.stream_ptr()))
        return out

    def resample_vjp(self, g_y, out=None):
        """Adjoint of ``resample``: [B, n_y] -> [B, n_samp]."""
        if g_y.dim() != 2 or g_y.shape[1] != self.n_y or g_y.dtype != torch.float32 or not g_y.is_contiguous():
            raise ValueError(f"g_y must be contiguous float32 [B, {self.n_y}]")
        if out is None:
            out = torch.empty(g_y.shape[0], self.n_samp, device=self.device)
        N.check(N.lib.lipasr_mfcc_plan_resample_vjp(self._plan, N.ptr(g_y), g_y.shape[0], N.ptr(out), N.stream_ptr()))
        return out


_extractors = {}


def _extractor(sr_in, n_samp, batch_max):
    key = (sr_in, n_samp, torch.cuda.current_device())
    ex = _extractors.get(key)
    if ex is None or ex.batch_max < batch_max or ex._plan is None or not ex.h.alive:
        if len(_extractors) >= 8:  # plans hold ~0.1 MB per clip of batch_max: keep a handful
            _extractors.pop(next(iter(_extractors))).close()
        ex = MfccExtractor(sr_in, n_samp, batch_max)
        _extractors[key] = ex
    return ex


def mfcc(waveforms, sr_in=16000, utterance_length=STANDARD_UTTERANCE_LENGTH, n_valid=None):
    """Batched entry: [B, n] float32 or int16 PCM (tensor or array) at ``sr_in`` Hz -> device tensor [B, 20*utterance_length].
    n_valid ([B] ints): clips of different lengths, each row zero-padded (or not: the tail is ignored) to n."""
    dev = torch.device("cuda", torch.cuda.current_device())
    if torch.is_tensor(waveforms):
        w = waveforms
    else:
        a = np.asarray(waveforms)
        w = torch.as_tensor(a if a.dtype == np.int16 else a.astype(np.float32))
    if w.dtype != torch.int16:
        w = w.to(dtype=torch.float32)
    w = w.to(device=dev).contiguous()
    nv = None
    if n_valid is not None:
        nv = torch.as_tensor(np.asarray(n_valid, dtype=np.int32)).to(dev) if not torch.is_tensor(n_valid) else n_valid.to(device=dev, dtype=torch.int32)
    return _extractor(int(sr_in), w.shape[1], w.shape[0])(w, utterance_length, n_valid=nv)


def read_wav(file_path, pcm16=False):
    """librosa.load's decode + mono mix (float32 in [-1, 1)); returns (samples, sampling_rate).
    pcm16=True: a 16-bit mono file comes back as its raw int16 samples (the device scales them by 2^-15 while it stages
    them, lipasr_mfcc_i16: half the bytes over PCIe and from HBM); any other file still comes back as float32."""
    with wave.open(str(file_path), "rb") as f:
        sr, nch, width, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
        raw = f.readframes(n)
    if pcm16 and width == 2 and nch == 1:
        return np.frombuffer(raw, dtype="<i2").copy(), sr
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"unsupported sample width {width} in {file_path}")
    if nch > 1:
        x = x.reshape(-1, nch).mean(axis=1).astype(np.float32)
    return x, sr


def extract_features(file_path, utterance_length):
    """Reference :24-39: MFCC(20 x utterance_length) of one wav file, float32 NumPy."""
    x, sr = read_wav(file_path)
    out = mfcc(x[None, :], sr, utterance_length)
    return out.view(N_MFCC, utterance_length).cpu().numpy()


def compute_mfcc_all_files(filenames, chunk=512):
    """Reference :144-150: (N, 880) float64.  Files are decoded on the host (16-bit mono files stay int16) and go to the
    device in chunks of ``chunk`` clips of ANY lengths: one launch per chunk, each clip processed with its own length
    (n_valid), rows padded to the chunk's longest clip rounded up to a multiple of 4000 samples so that a corpus of
    one-second clips uses one plan."""
    feats = np.zeros((len(filenames), N_MFCC * STANDARD_UTTERANCE_LENGTH))
    by_sr = {}
    for i, fn in enumerate(filenames):
        x, sr = read_wav(fn, pcm16=True)
        by_sr.setdefault((sr, x.dtype == np.int16), []).append((i, x))
    for (sr, is_pcm), items in by_sr.items():
        ragged_ok = sr in (16000, 8000)  # the rates whose plans take per-clip lengths; other rates: one launch per distinct length
        if ragged_ok:
            batches = [items[s:s + chunk] for s in range(0, len(items), chunk)]
        else:
            groups = {}
            for it in items:
                groups.setdefault(len(it[1]), []).append(it)
            batches = [g[s:s + chunk] for g in groups.values() for s in range(0, len(g), chunk)]
        for b in batches:
            lens = np.array([len(x) for _, x in b], dtype=np.int32)
            n_max = int(lens.max())
            n_pad = -(-n_max // 4000) * 4000 if ragged_ok else n_max
            w = np.zeros((len(b), n_pad), dtype=np.int16 if is_pcm else np.float32)
            for r, (_, x) in enumerate(b):
                w[r, :len(x)] = x
            f = mfcc(w, sr, STANDARD_UTTERANCE_LENGTH, n_valid=lens if ragged_ok else None).cpu().numpy()
            for (i, _), row in zip(b, f):
                feats[i] = row
    return feats


# ------------------------------------------------------------------------------------------------ Lipschitz read-outs
def _dense_kernels(model):
    if isinstance(model, Model):
        return model.dense_kernels()
    dev = torch.device("cuda", torch.cuda.current_device())
    return [torch.as_tensor(np.asarray(l.get_weights()[0], dtype=np.float32)).to(dev).contiguous() for l in model.layers if "dense" in l.name]


def get_norms(model, iters=64):
    """Reference :154-161: sigma_max of every Dense kernel (power iteration on the device)."""
    ks = _dense_kernels(model)
    dev = ks[0].device
    h = N.get_handle(dev.index)
    out = torch.zeros(len(ks), device=dev)
    for i, k in enumerate(ks):
        v = torch.zeros(k.shape[1], device=dev)
        N.check(N.lib.lipasr_sigma_max(h.h, N.ptr(k), k.shape[0], k.shape[1], N.ptr(v), 0, iters, 0, N.ptr(out[i:i + 1]), N.stream_ptr()))
    return out.cpu().numpy().astype(np.float64)


def get_upper_lipschitz(norms):
    """Reference :165-166."""
    return np.prod(norms)


def product_norm(model):
    """||W_m^T ... W_1^T||_2 as a device scalar tensor."""
    ks = _dense_kernels(model)
    dev = ks[0].device
    h = N.get_handle(dev.index)
    sig = torch.zeros(1, device=dev)
    ptrs = N.ptr_array([k.data_ptr() for k in ks])
    N.check(N.lib.lipasr_product_norm(h.h, C.cast(ptrs, N.PV), N.int_array([k.shape[0] for k in ks]), N.int_array([k.shape[1] for k in ks]),
                                      len(ks), N.ptr(sig), N.stream_ptr()))
    return sig


def get_lipschitz_constrained(model):
    """Reference :169-196: product norm divided by prod over BatchNorm layers of max_j sqrt(var_j)/gamma_j."""
    sig = product_norm(model)
    dev = sig.device
    h = N.get_handle(dev.index)
    factors = []
    for layer in model.layers:
        if "batch" in layer.name:
            if isinstance(model, Model):
                gamma, _, _, var = layer._tensors()
            else:
                ws = layer.get_weights()
                gamma = torch.as_tensor(np.asarray(ws[0], dtype=np.float32)).to(dev)
                var = torch.as_tensor(np.asarray(ws[3], dtype=np.float32)).to(dev)
            f = torch.zeros(1, device=dev)
            N.check(N.lib.lipasr_bn_correction(h.h, N.ptr(gamma), N.ptr(var), gamma.numel(), N.ptr(f), N.stream_ptr()))
            factors.append(f)
    cst = float(sig.item())
    correction = float(np.prod([float(f.item()) for f in factors])) if factors else 1.0
    return cst / correction


# The read-outs above are global bounds taken from the weights.  The two below measure what the network does at given inputs:
# sigma_b = ||J_b||_2, J_b[c][k] = d out_c(x_b) / d x_b[k] in inference mode ("Local Lipschitz read-out").
JACOBIAN_CHUNK_BYTES = 256 << 20  # get_local_lipschitz keeps one chunk's Jacobian under this


def jacobian_sigma(jac, return_vectors=False):
    """Spectral norm of every [classes, n] slice of a float32 device tensor [B, classes, n] (lipasr_jacobian_sigma; any strides
    along the first two dimensions, e.g. a permuted view of class-major storage; classes <= 32) -> sigma [B] on the device.
    return_vectors=True: (sigma, u [B, classes], v [B, n]), the unit left and right singular vectors, the component of u of
    largest magnitude positive; v is the input direction along which the output moves fastest.  A slice of zeros gives 0 and zero
    vectors, a slice with a NaN or inf gives sigma = NaN for that sample alone."""
    if not torch.is_tensor(jac) or not jac.is_cuda or jac.dtype != torch.float32 or jac.dim() != 3:
        raise ValueError("jac must be a float32 device tensor [B, classes, n]")
    b, c, n = jac.shape
    if n > 1 and jac.stride(2) != 1:
        raise ValueError("jac must be contiguous along its last dimension")
    h = N.get_handle(jac.device.index)
    sigma = torch.empty(b, device=jac.device)
    u = torch.empty(b, c, device=jac.device) if return_vectors else None
    v = torch.empty(b, n, device=jac.device) if return_vectors else None
    N.check(N.lib.lipasr_jacobian_sigma(h.h, N.ptr(jac), b, c, n, jac.stride(0), jac.stride(1), N.ptr(sigma), N.ptr(u), N.ptr(v),
                                        N.stream_ptr()))
    return (sigma, u, v) if return_vectors else sigma


def get_local_lipschitz(estimator, x, on_logits=True, lengths=None, return_vectors=False):
    """The local Lipschitz constant of ``estimator`` at every row of ``x``: the largest singular value of the Jacobian of its logits
    (on_logits=True) or of its softmax probabilities w.r.t. the row -> float64 NumPy [B]; return_vectors=True: (sigma, u [B,
    classes], v [B, n]).  ``estimator``: a TensorFlowV2Classifier (rows of MFCC features) or a WaveformClassifier (rows of audio;
    ``lengths`` as there) of lipasr.estimators -- or anything with ``jacobian_device(xt, on_logits=)`` and ``nb_classes``, which is
    why ``lengths`` is passed on only when given and ``batch_limit`` used only where there is one.  Rows go through in chunks of
    the batch limit, cut further so that one chunk's Jacobian stays under JACOBIAN_CHUNK_BYTES."""
    xt = E._to_dev(x)
    if xt.dim() != 2:
        raise ValueError(f"x must be [B, n], got {tuple(xt.shape)}")
    b, n = xt.shape
    c = int(estimator.nb_classes)
    chunk = max(1, JACOBIAN_CHUNK_BYTES // max(1, 4 * c * n))
    chunk = min(chunk, int(getattr(estimator, "batch_limit", None) or chunk))
    sig, us, vs = [], [], []
    for s in range(0, b, chunk):
        kw = {} if lengths is None else {"lengths": lengths[s:s + chunk]}
        jac = estimator.jacobian_device(xt[s:s + chunk], on_logits=on_logits, **kw)
        r = jacobian_sigma(jac, return_vectors)
        if return_vectors:
            sig.append(r[0]); us.append(r[1]); vs.append(r[2])
        else:
            sig.append(r)
    cat = lambda parts, shape: (torch.cat(parts).double().cpu().numpy() if parts else np.zeros(shape))
    if return_vectors:
        return cat(sig, (0,)), cat(us, (0, c)), cat(vs, (0, n))
    return cat(sig, (0,))


# The two below turn those constants into distances ("Robustness radius"): per row, how far the decision boundary is at
# least (certified, from the global bound), how far its linearisation is, and how far DeepFool had to go.
def get_lipschitz_bound(model):
    """A true upper bound of the Lipschitz constant of the model's logits in the 2-norm ("Local Lipschitz read-out"):
    prod_l ||W_l||_2 (get_norms) x prod over BatchNorm layers of max_j |gamma_j| / sqrt(var_j + 1e-3).  get_lipschitz_constrained,
    the reference's read-out, is not a bound (it divides by max_j sqrt(var_j) / gamma_j).  The power iteration of get_norms comes
    to ||W_l||_2 from below, and from its fixed positive start the default 64 round trips leave a signed kernel's product up to
    2 % short (non-negative kernels have a dominant singular vector and are there long before); 1024 leave 2e-7 on the worst
    kernels the tests have."""
    bound = float(np.prod(get_norms(model, iters=1024)))
    for layer in model.layers:
        if "batch" in layer.name:
            ws = [np.asarray(w, dtype=np.float64) for w in layer.get_weights()]
            bound *= float(np.max(np.abs(ws[0]) / np.sqrt(ws[3] + 1e-3)))
    return bound


def get_robustness_radius(estimator, x, norm=2, lengths=None, smoothing=None, found_by="deepfool", bounds=None, **attack_kw):
    """Per row of ``x`` the three numbers  certified radius <= distance to the decision boundary <= distance DeepFool found,  as a
    dict of float64 NumPy arrays [B]:
      margin     min over k != c of z_c - z_k on the logits, c the estimator's own class at the row;
      certified  margin / (sqrt(2) L), L = get_lipschitz_bound(model): no point closer than this is classified differently
                 (z_c - z_k has the Lipschitz constant ||e_c - e_k||_2 L).  Given for rows of features (TensorFlowV2Classifier)
                 and norm 2 only; None over audio (the log of the MFCC stage has no global constant) and for norm inf;
      linear     the distance to the nearest boundary of the classifier linearised at the row (DeepFool's first rho_l);
      found      ||x_adv - x|| in ``norm`` for attacks.DeepFool(estimator, norm=norm, **attack_kw);
      flipped    bool: x_adv is classified differently.  Where it is False, ``found`` bounds nothing.
    ``found_by``: "deepfool" (default), or "hopskipjump": ``found`` and ``flipped`` then come from attacks.HopSkipJump(estimator,
    norm=norm, **attack_kw) -- its ``distance_`` (+inf without a start) and ``success_`` -- a distance that rests on the label alone,
    neither on a gradient nor on a score, next to the same margin, certified radius and linearised distance (ONE DeepFool step
    with its default keywords: ``attack_kw`` are HopSkipJump's then).
    ``smoothing``: None (default: the dict above, nothing else), or dict(sigma=, n0=100, n=100_000, alpha=0.001, seed=0,
    clip_values=None) -- randomized smoothing (lipasr.smoothing.Smooth.certify) then adds
      smoothed_radius  the L2 radius sigma Phi^-1(p_lower) within which the SMOOTHED classifier g(x) = argmax_c P(f(x + N(0,
                       sigma^2 I)) = c) keeps its class, with probability 1 - alpha over the draws; 0 where it abstains;
      smoothed_class   int64: the class of g at the row, -1 where it abstains.
    It certifies the smoothed classifier, not the base one whose margin, ``certified`` and ``found`` stand next to it; over audio
    and for a model without a useful Lipschitz bound it is the only certified entry.  It is an L2 radius whatever ``norm`` is.
    ``bounds``: None (default: nothing is added), or dict(eps_max=1.0, steps=12, method="crown-ibp") -- bound propagation
    (lipasr.bounds.certified_radius) then adds
      bound_radius     in the call's ``norm`` (2 or inf): the largest eps of a bisection on [0, eps_max] at which IBP / CROWN-IBP
                       certify the BASE classifier's own class over the whole ball; deterministic, and the only certified entry
                       in norm inf.  Rows of features only: a WaveformClassifier is refused, as lipasr.bounds refuses it.
    ``estimator``: a TensorFlowV2Classifier or WaveformClassifier of lipasr.estimators (``lengths`` as there)."""
    from .attacks import DeepFool  # attacks imports this module

    if found_by not in ("deepfool", "hopskipjump"):
        raise ValueError(f"found_by = {found_by!r}: 'deepfool' or 'hopskipjump'")
    xt = E._to_dev(x)
    attack = DeepFool(estimator, norm=norm, max_iter=1) if found_by == "hopskipjump" else DeepFool(estimator, norm=norm, **attack_kw)
    if xt.shape[0] == 0:
        z = torch.zeros(0, estimator.nb_classes, device=xt.device)
    else:
        z = estimator.predict_device(xt, logits=True, lengths=lengths)
    z = z.double()
    if z.shape[1] > 1:
        top = torch.topk(z, 2, dim=1).values
        margin = (top[:, 0] - top[:, 1]).cpu().numpy()
    else:
        margin = np.full(z.shape[0], np.inf)
    adv = attack.generate_device(xt, lengths=lengths)
    d = (adv - xt).double()
    found = (d.pow(2).sum(dim=1).sqrt() if attack.norm == 2.0 else d.abs().amax(dim=1)).cpu().numpy()
    certified = None
    # the model's bound speaks about the estimator where its rows are the model's own inputs: no extraction stage in front
    if getattr(estimator, "extractor", None) is None and attack.norm == 2.0:
        certified = margin / (np.sqrt(2.0) * get_lipschitz_bound(estimator.model))
    res = {"margin": margin, "certified": certified, "linear": attack.last["first_dist"], "found": found,
           "flipped": attack.last["flipped"]}
    if found_by == "hopskipjump":
        from .attacks import HopSkipJump

        hsj = HopSkipJump(estimator, norm=norm, **attack_kw)
        hsj.generate_device(xt, lengths=lengths)
        res["found"], res["flipped"] = hsj.distance_.double().cpu().numpy(), hsj.success_.cpu().numpy()
    if smoothing is not None:
        from .smoothing import Smooth

        kw = dict(smoothing)
        if "sigma" not in kw:
            raise ValueError("smoothing= needs sigma")
        sm = Smooth(estimator, kw.pop("sigma"), seed=kw.pop("seed", 0), clip_values=kw.pop("clip_values", None))
        cert = sm.certify(xt, lengths=lengths, **kw)
        res["smoothed_radius"], res["smoothed_class"] = cert["radius"], cert["class"]
    if bounds is not None:
        from .bounds import certified_radius

        res["bound_radius"] = certified_radius(estimator, xt, norm=norm, **dict(bounds)).double().cpu().numpy()
    return res


# ------------------------------------------------------------------------------------------------ dataset construction
digit = ['zero', 'one', 'two', 'three', 'four', 'five', 'six', 'seven', 'eight', 'nine']  # reference :120


def get_file_names_and_labels(file_path, classes=None):
    """Reference :118-141: the class folders of ``file_path`` that exist (in the order of ``digit``), every file in
    them, and one integer label per file -- the label is the folder's rank among the folders that are PRESENT."""
    import glob
    import os

    classes = digit if classes is None else classes
    present = set(os.listdir(str(file_path)))
    filenames, labels = [], []
    for i, name in enumerate([c for c in classes if c in present]):
        found = sorted(glob.glob(os.path.join(str(file_path), name, "*")))
        filenames += found
        labels += [i] * len(found)
    return filenames, np.array(labels)


def shuffle(*arrays, random_state=None):
    """sklearn.utils.shuffle (reference :205): one permutation applied to every argument; lists stay lists."""
    if not arrays:
        return None
    n = len(arrays[0])
    if any(len(a) != n for a in arrays):
        raise ValueError("shuffle: arguments of different lengths")
    rng = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    perm = rng.permutation(n)
    out = [[a[i] for i in perm] if isinstance(a, (list, tuple)) else np.asarray(a)[perm] for a in arrays]
    return out[0] if len(out) == 1 else out


def split_train_dev_test(items):
    """Reference :208-214: [:0.7 n], [0.7 n : 0.9 n], [-0.1 n:] with the reference's int() truncations (for n < 10 the
    last slice is ``[-0:]``, i.e. everything, exactly as the reference's expression evaluates)."""
    n = len(items)
    a, b, c = int(n * 0.7), int(n * 0.9), int(n * 0.1)
    return items[:a], items[a:b], items[-c:]


def main(data_dir="data", save_dir="processed_google_dataset", noise_dir="test_dataset_to_add_noise", random_state=None):
    """Reference :198-232 (the ``__main__`` block): list, shuffle, split 70/20/10, MFCC of every file on the GPU,
    and the eight ``.npy`` files train_constraints.py:16-25 and attacks.py read."""
    import os

    filenames, labels = get_file_names_and_labels(data_dir)
    filenames, labels = shuffle(filenames, labels, random_state=random_state)
    filenames_train, filenames_dev, filenames_test = split_train_dev_test(filenames)
    labels_train, labels_dev, labels_test = split_train_dev_test(labels)
    os.makedirs(noise_dir, exist_ok=True)
    os.makedirs(save_dir, exist_ok=True)
    np.save(os.path.join(noise_dir, "test_label"), labels_test)
    np.save(os.path.join(noise_dir, "test_filenames"), filenames_test)
    for name, files, lab in (("train", filenames_train, labels_train), ("dev", filenames_dev, labels_dev),
                             ("test", filenames_test, labels_test)):
        np.save(os.path.join(save_dir, f"{name}_data"), compute_mfcc_all_files(files))
        np.save(os.path.join(save_dir, f"{name}_label"), lab)
    return save_dir


if __name__ == "__main__":
    main()
