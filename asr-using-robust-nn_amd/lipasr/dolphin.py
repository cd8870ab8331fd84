"""DolphinAttack ("Voice digit recogniton/dolphin_attack.m"): a 16 kHz voice command as inaudible amplitude-modulated
ultrasound at 192 kHz, and the clip a microphone with a quadratic non-linearity records from it.

    band-pass 100 Hz - 7 kHz (Butterworth order 10, ten biquads) -> x12 (MATLAB resample's filter) -> / max|.|
    -> (u + carrier_level) cos(2 pi carrier_hz k / 192000) -> / max|.|          [the ultrasound; the script ends here]
    -> a1 s + a2 s^2 -> /12 with the same filter                                [the microphone model]

Every step is a kernel behind the C ABI (lipasr_dolphin_* in include/lipasr.h, which has the equations); this module only
owns the plan and hands device tensors through.  ``generate_recorded`` runs the whole chain with the 192 kHz signal kept in
LDS: its result is a 16 kHz clip as long as the input, ready for MfccExtractor with the same ``n_valid``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N

RATIO = 12  # 192 kHz / 16 kHz


class DolphinAttack:
    """One native plan for clips of up to ``n_samp_max`` samples at ``sr`` Hz (16 000 only), ``batch_max`` clips per launch.
    ``carrier_level`` is the constant added to the normalised voice before the carrier multiplies it: 0.001 is the
    reference script's (the recorded clip is then essentially the voice squared), 1 the DolphinAttack paper's."""

    def __init__(self, sr=16000, n_samp_max=16000, batch_max=64, carrier_hz=30000, carrier_level=0.001, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.h = N.get_handle(self.device.index)
        self.sr, self.n_samp_max, self.batch_max = int(sr), int(n_samp_max), int(batch_max)
        self.carrier_hz, self.carrier_level = float(carrier_hz), float(carrier_level)
        plan = N.c_h()
        N.check(N.lib.lipasr_dolphin_create(self.h.h, self.sr, self.n_samp_max, self.batch_max, self.carrier_hz, self.carrier_level,
                                            C.byref(plan)))
        self._plan = plan
        N.register_owner(self)

    def close(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan and self.h.alive:
            N.destroy_or_defer(N.lib.lipasr_dolphin_destroy, plan)  # (a finaliser may run in the middle of a graph capture)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, x, width, what):
        if self._plan is None:
            raise RuntimeError("DolphinAttack used after close()")
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != width \
                or not x.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 device tensor [B, {width}]")
        return x.shape[0]

    def _lengths(self, lengths, b):
        if lengths is None:
            return None
        if not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (b,) or not lengths.is_cuda \
                or not lengths.is_contiguous():
            raise ValueError(f"lengths must be a contiguous int32 device tensor [{b}]")
        return lengths

    def bandpass(self, x, lengths=None, out=None):
        """[B, n_samp_max] -> the band-passed voice [B, n_samp_max] (zeros from each clip's length on)."""
        b = self._rows(x, self.n_samp_max, "x")
        v = torch.empty_like(x) if out is None else out
        N.check(N.lib.lipasr_dolphin_bandpass(self._plan, N.ptr(x), N.ptr(self._lengths(lengths, b)), b, N.ptr(v), N.stream_ptr()))
        return v

    def generate(self, x, lengths=None, return_peaks=False):
        """[B, n_samp_max] -> the ultrasound [B, 12 n_samp_max] at 192 kHz, peak 1 (and the two maxima [B, 2] on request)."""
        b = self._rows(x, self.n_samp_max, "x")
        s = torch.empty(b, RATIO * self.n_samp_max, device=self.device)
        peaks = torch.empty(b, 2, device=self.device) if return_peaks else None
        N.check(N.lib.lipasr_dolphin_generate(self._plan, N.ptr(x), N.ptr(self._lengths(lengths, b)), b, N.ptr(s), N.ptr(peaks),
                                              N.stream_ptr()))
        return (s, peaks) if return_peaks else s

    def record(self, ultra, a1=1.0, a2=0.5, lengths=None):
        """Any 192 kHz buffer [B, 12 n_samp_max] -> what the microphone a1 s + a2 s^2 records at 16 kHz, [B, n_samp_max].
        ``lengths`` counts 16 kHz samples."""
        b = self._rows(ultra, RATIO * self.n_samp_max, "ultra")
        r = torch.empty(b, self.n_samp_max, device=self.device)
        N.check(N.lib.lipasr_dolphin_record(self._plan, N.ptr(ultra), N.ptr(self._lengths(lengths, b)), b, float(a1), float(a2),
                                            N.ptr(r), N.stream_ptr()))
        return r

    def generate_recorded(self, x, lengths=None, a1=1.0, a2=0.5, out=None):
        """generate followed by record in one pass that never stores the 192 kHz signal: [B, n_samp_max] -> [B, n_samp_max]."""
        b = self._rows(x, self.n_samp_max, "x")
        r = torch.empty_like(x) if out is None else out
        N.check(N.lib.lipasr_dolphin_generate_recorded(self._plan, N.ptr(x), N.ptr(self._lengths(lengths, b)), b, float(a1), float(a2),
                                                       N.ptr(r), N.stream_ptr()))
        return r

    def generate_wav(self, x):
        """NumPy convenience: one clip [n] or clips [B, n] (n <= n_samp_max) -> the 192 kHz ultrasound, [12 n] or [B, 12 n]."""
        a = np.asarray(x, dtype=np.float32)
        one = a.ndim == 1
        a = a[None, :] if one else a
        if a.ndim != 2 or a.shape[1] > self.n_samp_max:
            raise ValueError(f"x must be [n] or [B, n] with n <= {self.n_samp_max}")
        out = np.zeros((a.shape[0], RATIO * a.shape[1]), dtype=np.float32)
        for s0 in range(0, a.shape[0], self.batch_max):
            rows = np.zeros((min(self.batch_max, a.shape[0] - s0), self.n_samp_max), dtype=np.float32)
            rows[:, :a.shape[1]] = a[s0:s0 + rows.shape[0]]
            lens = torch.full((rows.shape[0],), a.shape[1], dtype=torch.int32, device=self.device)
            s = self.generate(torch.as_tensor(rows).to(self.device), lens)
            out[s0:s0 + rows.shape[0]] = s[:, :RATIO * a.shape[1]].cpu().numpy()
        return out[0] if one else out
