"""The estimators the attacks and read-outs run over, and the one device-side surface they share.

``TensorFlowV2Classifier`` (ART's wrapper, attacks.py:500-504) takes rows of MFCC features, the model's own inputs;
``WaveformClassifier`` (ours) puts the MFCC stage in front of the model and takes rows of audio; ``OverTheAirClassifier`` (ours) puts
a bank of room impulse responses (lipasr.room.RoomChannel) in front of a WaveformClassifier and answers with the expectation over
the rooms, so that every attack over audio has an over-the-air form; ``DefendedClassifier`` (ours) puts an input-transformation
defence (lipasr.defences.AudioDefence: median, FIR and bit-depth stages) in front of a WaveformClassifier, so that every attack over
audio has an adaptive form against it.  All answer the same calls on device tensors, so that an attack
asks its estimator and never what kind of estimator it holds:

    model, nb_classes, input_shape, batch_limit, clip_values (None: no clamp -- always on a TensorFlowV2Classifier)
    rows_device(x)                                  x as the float32 device tensor [B, input_shape[0]]
    lengths_device(lengths, b)                      per-clip lengths as the int32 device tensor [b]; None stays None, and only an
                                                    estimator over audio takes anything else (with it: clip_mask(lt))
    predict_device(xt, logits=False, lengths=None)
    own_labels_device(xt, lengths=None, batch=None) one-hot of the estimator's own predictions (lipasr_mlp_own_labels)
    loss_gradient_device(xt, yt, out=None, lengths=None)
    output_vjp_device(xt, vt, on_logits=False, ..., lengths=None)
    jacobian_device(xt, on_logits=True, ..., lengths=None)
    predict_each_device(xt, lengths=None, logits=False)   OverTheAirClassifier only: [B, R, classes], every room on its own

``lipasr.attacks`` re-exports every name of this module.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from . import extract_features_construct_dataset as X  # the module, not its names: it imports this one for its read-outs
from .keras import Model


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(x):
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    return t.to(device=_dev(), dtype=torch.float32).contiguous()


def _as_given(adv, x):
    """NumPy in, NumPy out: the device tensor ``adv`` itself where ``x`` came as a tensor, else its NumPy copy in ``x``'s dtype."""
    return adv if torch.is_tensor(x) else adv.cpu().numpy().astype(np.asarray(x).dtype, copy=False)


class _Estimator:
    """What TensorFlowV2Classifier and WaveformClassifier share (the module docstring lists the surface).  A subclass sets
    ``input_shape`` and gives predict_device, loss_gradient_device, output_vjp_device and jacobian_device; one with a stage in front
    of the model also gives ``_features`` and its own ``lengths_device``."""

    clip_values = None

    def __init__(self, model, nb_classes):
        if not isinstance(model, Model):
            raise TypeError("model must be a lipasr.keras.Model")
        self.model, self.nb_classes = model, int(nb_classes)

    @property
    def batch_limit(self):
        """Rows one native call takes (the model's max_batch)."""
        return self.model._max_batch

    def rows_device(self, x):
        """``x`` (array or tensor) as the contiguous float32 device tensor [B, input_shape[0]] every other call takes."""
        xt = _to_dev(x)
        if xt.dim() != 2 or xt.shape[1] != self.input_shape[0]:
            raise ValueError(f"x must be [B, {self.input_shape[0]}], got {tuple(xt.shape)}")
        return xt

    def lengths_device(self, lengths, b):
        """Rows of features have no per-clip lengths: None stays None, anything else is refused."""
        if lengths is not None:
            raise ValueError("lengths= is for attacks over audio: the estimator must be a WaveformClassifier")
        return None

    def _features(self, xb, lb):
        """The model's input for the rows ``xb`` (at most batch_limit of them): the rows themselves."""
        return xb

    def own_labels_device(self, xt, lengths=None, batch=None):
        """One-hot [B, classes] of the estimator's own predictions at ``xt``: ONE lipasr_mlp_own_labels per chunk of
        min(batch, batch_limit) rows, over audio on the features of the chunk."""
        m = self.model
        bs = min(batch or self.batch_limit, self.batch_limit)
        lt = self.lengths_device(lengths, xt.shape[0])
        yt = torch.empty(xt.shape[0], self.nb_classes, device=xt.device)
        for s in range(0, xt.shape[0], bs):
            f = self._features(xt[s:s + bs], None if lt is None else lt[s:s + bs])
            N.check(N.lib.lipasr_mlp_own_labels(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(f), f.shape[0], N.ptr(yt[s:s + bs]),
                                                N.stream_ptr()))
        return yt

    def loss_gradient(self, x, y, lengths=None):
        """d mean CE(f(x), y) / dx in inference mode, NumPy in / NumPy out."""
        return self.loss_gradient_device(_to_dev(x), _to_dev(y), lengths=lengths).cpu().numpy()


# ------------------------------------------------------------------------------------------------ A9 / A10
class TensorFlowV2Classifier(_Estimator):
    """ART estimator wrapper (attacks.py:500-504): ``predict`` and ``loss_gradient`` over a lipasr Model."""

    def __init__(self, model, nb_classes, input_shape, loss_object=None, clip_values=None):
        super().__init__(model, nb_classes)
        if clip_values is not None:
            raise NotImplementedError("the reference passes no clip_values")
        self.input_shape = tuple(input_shape)
        if model._n_classes != self.nb_classes or model._widths[0] != self.input_shape[0]:
            raise ValueError("nb_classes / input_shape do not match the model")

    def predict(self, x, batch_size=128):
        return self.model.predict(x)

    def predict_device(self, xt, logits=False, lengths=None):
        self.lengths_device(lengths, xt.shape[0])
        return self.model.predict_device(xt, logits=logits)

    def loss_gradient_device(self, xt, yt, out=None, lengths=None):
        """d mean CE(f(x), y) / dx on device tensors ([B, features], one-hot [B, classes]) -> [B, features]."""
        self.lengths_device(lengths, xt.shape[0])
        m = self.model
        out = torch.empty_like(xt) if out is None else out
        bs = m._max_batch
        for s in range(0, xt.shape[0], bs):
            xb, yb, ob = xt[s:s + bs], yt[s:s + bs], out[s:s + bs]
            N.check(N.lib.lipasr_mlp_input_grad(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xb), N.ptr(yb), xb.shape[0], N.ptr(ob), N.stream_ptr()))
        return out

    def output_vjp_device(self, xt, vt, on_logits=False, probs_out=None, lengths=None):
        """sum_c v[b, c] d out_c / dx on device tensors ([B, features], [B, classes]) -> [B, features]."""
        self.lengths_device(lengths, xt.shape[0])
        m = self.model
        out = torch.empty_like(xt)
        bs = m._max_batch
        for s in range(0, xt.shape[0], bs):
            xb, vb, ob = xt[s:s + bs], vt[s:s + bs], out[s:s + bs]
            pb = None if probs_out is None else probs_out[s:s + bs]
            N.check(N.lib.lipasr_mlp_output_vjp(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xb), N.ptr(vb), 1 if on_logits else 0,
                                                xb.shape[0], N.ptr(pb), N.ptr(ob), N.stream_ptr()))
        return out

    def jacobian_device(self, xt, on_logits=True, probs_out=None, lengths=None):
        """d out_c / dx for every class on a device tensor [B, features] -> [B, classes, features] (lipasr_mlp_jacobian: ONE forward
        pass per batch, then one backward chain per class; row c is what ``output_vjp_device`` gives for the one-hot vector e_c).
        probs_out: optional [B, classes] tensor that receives softmax(f(x))."""
        self.lengths_device(lengths, xt.shape[0])
        m = self.model
        xt = xt.contiguous()
        c, n = self.nb_classes, xt.shape[1]
        out = torch.empty(xt.shape[0], c, n, device=xt.device)
        bs = m._max_batch
        for s in range(0, xt.shape[0], bs):
            xb, ob = xt[s:s + bs], out[s:s + bs]
            pb = None if probs_out is None else probs_out[s:s + bs]
            N.check(N.lib.lipasr_mlp_jacobian(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xb), 1 if on_logits else 0, xb.shape[0],
                                              N.ptr(pb), N.ptr(ob), c * n, n, N.stream_ptr()))
        return out

    def class_gradient(self, x, label=None):
        """ART class_gradient: gradients of the model OUTPUT (softmax probabilities) w.r.t. x.
        label None -> [B, nb_classes, features]; int or int array [B] -> [B, 1, features]."""
        xt = _to_dev(x)
        b = xt.shape[0]
        if label is None:
            cols = []
            for c in range(self.nb_classes):
                v = torch.zeros(b, self.nb_classes, device=xt.device)
                v[:, c] = 1.0
                cols.append(self.output_vjp_device(xt, v))
            return torch.stack(cols, dim=1).cpu().numpy()
        lab = torch.as_tensor(np.broadcast_to(np.asarray(label), (b,)).astype(np.int64), device=xt.device)
        v = torch.zeros(b, self.nb_classes, device=xt.device)
        v[torch.arange(b, device=xt.device), lab] = 1.0
        return self.output_vjp_device(xt, v)[:, None, :].cpu().numpy()


class WaveformClassifier(_Estimator):
    """Estimator over audio: waveform -> MFCC (K1) -> optional StandardScaler affine -> model.  ``loss_gradient`` follows
    TensorFlowV2Classifier.loss_gradient's convention (lipasr_mlp_input_grad: d mean CE / d features in inference mode) and
    carries it to the samples with the backward pass of the MFCC stage (MfccExtractor.vjp).
    domain="22k" (default): the input is the 22 050 Hz signal [B, extractor.n_y], what the reference's audio noise attacks
    perturb (librosa.load's output, attacks.py:108-114), so that black-box and white-box audio curves share an amplitude axis;
    domain="input": the file's samples [B, n_samp] at ``sr_in``.  ``mean`` / ``scale``: [20 * utterance_length] statistics
    fused into the extraction (both or neither).  ``clip_values``: the attacks clamp their iterates to it.
    ``lengths`` (features_device, predict*, loss_gradient*): int32 device tensor or array [B], the samples of each row that belong
    to its clip, counted at ``sr_in`` for EITHER domain (a 22 050 Hz row holds its clip in its first ceil(n * 22050 / sr_in)
    positions): clips of different lengths in one batch, each treated as if it were alone; the rest of a row is ignored and its
    gradient is exactly 0.  None: every row is a whole clip, and every call is the one made without the keyword.
    A short-window extractor (``MfccExtractor(..., n_fft=441, hop=220)``, the Speaker-recognition features) sends the gradient
    through ``MfccExtractor.vjp_short``; it has no per-clip lengths (``lengths=`` raises ValueError)."""

    def __init__(self, model, nb_classes, extractor=None, sr_in=16000, n_samp=16000, utterance_length=44, mean=None, scale=None,
                 domain="22k", clip_values=(-1.0, 1.0)):
        super().__init__(model, nb_classes)
        if domain not in ("22k", "input"):
            raise ValueError(f"domain={domain!r}: '22k' or 'input'")
        if (mean is None) != (scale is None):
            raise ValueError("give both mean and scale or neither")
        self.utterance_length, self.domain = int(utterance_length), domain
        self.extractor = extractor if extractor is not None else X.MfccExtractor(sr_in, n_samp, batch_max=model._max_batch, device=model._device)
        self.n = self.extractor.n_y if domain == "22k" else self.extractor.n_samp
        self.input_shape = (self.n,)
        n_feat = 20 * self.utterance_length
        if model._n_classes != self.nb_classes or model._widths[0] != n_feat:
            raise ValueError("nb_classes / utterance_length do not match the model")
        dev = self.extractor.device
        as64 = lambda v: None if v is None else torch.as_tensor(v).to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
        self.mean, self.scale = as64(mean), as64(scale)
        if self.mean is not None and (self.mean.numel() != n_feat or self.scale.numel() != n_feat):
            raise ValueError(f"mean and scale must have {n_feat} elements")
        self.clip_values = None if clip_values is None else (float(clip_values[0]), float(clip_values[1]))
        self._bs = min(model._max_batch, self.extractor.batch_max)

    @property
    def batch_limit(self):
        """Rows one native call takes (the smaller of the model's and the extractor's)."""
        return self._bs

    def lengths_device(self, lengths, b):
        """``lengths`` as the int32 device tensor [b] the extractor takes (None stays None)."""
        if lengths is None:
            return None
        if self.extractor.short_window:
            raise ValueError("lengths=: a short-window extractor takes rows of one length (there is no per-clip-length short-window path)")
        t = lengths if torch.is_tensor(lengths) else torch.as_tensor(np.asarray(lengths).astype(np.int32))
        t = t.to(device=self.extractor.device, dtype=torch.int32).contiguous()
        if tuple(t.shape) != (b,):
            raise ValueError(f"lengths must hold one sample count per row ([{b}]), got {tuple(t.shape)}")
        return t

    def clip_positions(self, lt):
        """int32 [B]: the positions of each row that belong to its clip -- its samples (domain "input"), or the ceil(n * 22050 /
        sr_in) positions the kernels derive from them (domain "22k", the same float64 expression as clip_lengths)."""
        ex = self.extractor
        n = lt.clamp(0, ex.n_samp)
        if self.domain == "22k":
            n = torch.ceil(n.to(torch.float64) * (22050.0 / float(ex.sr_in))).to(torch.int32)
        return n

    def clip_mask(self, lt):
        """bool [B, n]: the positions of each row inside its clip, [0, clip_positions)."""
        return torch.arange(self.n, device=lt.device, dtype=torch.int32)[None, :] < self.clip_positions(lt)[:, None]

    def features_device(self, xt, lengths=None):
        """[B <= batch_max, n] device tensor -> standardised features [B, 20 * utterance_length]."""
        if lengths is not None:
            lengths = self.lengths_device(lengths, xt.shape[0])
        if self.domain == "22k":
            return self.extractor.from_22k(xt, self.utterance_length, self.mean, self.scale, n_valid=lengths)
        return self.extractor(xt, self.utterance_length, self.mean, self.scale, n_valid=lengths)

    def _features(self, xb, lb):
        return self.features_device(xb.contiguous(), lb)

    def predict_device(self, xt, logits=False, lengths=None):
        xt = self.rows_device(xt)
        lt = self.lengths_device(lengths, xt.shape[0])
        return torch.cat([self.model.predict_device(self._features(xt[s:s + self._bs], None if lt is None else lt[s:s + self._bs]),
                                                    logits=logits)
                          for s in range(0, xt.shape[0], self._bs)])

    def predict(self, x, batch_size=128, lengths=None):
        return self.predict_device(_to_dev(x), lengths=lengths).cpu().numpy()

    def loss_gradient_device(self, xt, yt, out=None, lengths=None):
        """d mean CE(f(features(x)), y) / dx on device tensors ([B, n], one-hot [B, classes]) -> [B, n]."""
        xt = self.rows_device(xt)
        m = self.model
        out = torch.empty_like(xt) if out is None else out
        lt = self.lengths_device(lengths, xt.shape[0])
        for s in range(0, xt.shape[0], self._bs):
            xb, yb, ob = xt[s:s + self._bs], yt[s:s + self._bs], out[s:s + self._bs]
            lb = None if lt is None else lt[s:s + self._bs]
            f = self.features_device(xb, lb)
            gf = torch.empty_like(f)
            N.check(N.lib.lipasr_mlp_input_grad(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(f), N.ptr(yb), xb.shape[0], N.ptr(gf), N.stream_ptr()))
            self._features_vjp(xb, gf, lb, ob)
        return out

    def _features_vjp(self, xb, gf, lb, ob):
        """The feature cotangent ``gf`` carried back to the rows ``xb`` whose features this extractor has just computed (its last
        call on the current stream), into ``ob``: the backward pass that matches the extractor and ``lb``."""
        ex = self.extractor
        if ex.short_window:
            ex.vjp_short(xb, gf, self.utterance_length, self.scale, domain=self.domain, reuse_forward=True, out=ob)
        elif lb is None:
            ex.vjp(xb, gf, self.utterance_length, self.scale, domain=self.domain, reuse_forward=True, out=ob)
        else:
            ex.vjp_ragged(xb, gf, lb, self.utterance_length, self.scale, domain=self.domain, reuse_forward=True, out=ob)

    def output_vjp_device(self, xt, vt, on_logits=False, lengths=None):
        """sum_c v[b, c] d out_c / dx on device tensors ([B, n], [B, classes]) -> [B, n]: TensorFlowV2Classifier.output_vjp_device
        with the MFCC stage in front (extraction, lipasr_mlp_output_vjp, the backward pass of the extraction)."""
        xt = self.rows_device(xt)
        m = self.model
        vt = vt.contiguous()
        out = torch.empty_like(xt)
        lt = self.lengths_device(lengths, xt.shape[0])
        for s in range(0, xt.shape[0], self._bs):
            xb, vb, ob = xt[s:s + self._bs], vt[s:s + self._bs], out[s:s + self._bs]
            lb = None if lt is None else lt[s:s + self._bs]
            f = self.features_device(xb, lb)
            gf = torch.empty_like(f)
            N.check(N.lib.lipasr_mlp_output_vjp(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(f), N.ptr(vb), 1 if on_logits else 0,
                                                xb.shape[0], None, N.ptr(gf), N.stream_ptr()))
            self._features_vjp(xb, gf, lb, ob)
        return out

    def jacobian_device(self, xt, on_logits=True, lengths=None):
        """d out_c / dx for every class on a device tensor [B, n] -> a [B, classes, n] view of class-major storage.  Per batch: ONE
        extraction, ONE lipasr_mlp_jacobian into [classes][B][features] (the MFCC backward takes contiguous [B, features]
        cotangents), then one backward pass of the MFCC stage per class on the intermediates the extraction left: the backward
        chain only reads them, so they serve every class.  Row c carries the bits of ``output_vjp_device`` with the one-hot e_c."""
        xt = self.rows_device(xt)
        m = self.model
        b_all, c = xt.shape[0], self.nb_classes
        lt = self.lengths_device(lengths, b_all)
        out = torch.empty(c, b_all, self.n, device=xt.device)
        for s in range(0, b_all, self._bs):
            xb = xt[s:s + self._bs]
            lb = None if lt is None else lt[s:s + self._bs]
            f = self.features_device(xb, lb)
            b, nf = f.shape
            jf = torch.empty(c, b, nf, device=xt.device)
            N.check(N.lib.lipasr_mlp_jacobian(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(f), 1 if on_logits else 0, b, None,
                                              N.ptr(jf), nf, b * nf, N.stream_ptr()))
            for k in range(c):
                self._features_vjp(xb, jf[k], lb, out[k, s:s + b])
        return out.permute(1, 0, 2)


class OverTheAirClassifier(WaveformClassifier):
    """A WaveformClassifier heard through rooms: every clip goes through each of the R room impulse responses of a
    lipasr.room.RoomChannel before the MFCC stage, and the estimator answers with the expectation over the rooms (expectation over
    transformations, the robustness half of Qin et al. 2019).  It shares the base's model, extractor, statistics, domain and
    ``clip_values`` and takes the same rows, so any attack over audio runs on it unchanged; the responses are applied to the rows
    as they come, so their sample rate has to be the rows' (22 050 Hz in domain "22k"): that is the caller's business.
    ``lengths`` keep the base's meaning (samples at ``sr_in``); the channel cuts the reverberant tail at the clip's end, so they hold
    behind it too, and the gradient stays exactly 0 beyond each clip.
        predict_device        the mean over the rooms of the base's probabilities (or logits)
        predict_each_device   [B, R, classes], every room on its own: the evaluation read-out
        loss_gradient_device  d mean_{b, j} CE / dx: the base's gradient at the B R expanded rows (its mean over a chunk's rows already
                              averages over the rooms) carried back through the channel and summed over the rooms
        output_vjp_device, jacobian_device   the mean over the rooms of the base's
        own_labels_device     the base's: the prediction on the DRY clip, which is what was said
    One native call of the base takes c R rows, so ``batch_limit`` is the base's divided by R (in clips)."""

    def __init__(self, base, channel):
        from .room import RoomChannel

        if not isinstance(base, WaveformClassifier) or isinstance(base, OverTheAirClassifier):
            raise TypeError("base must be a WaveformClassifier (and not itself an OverTheAirClassifier)")
        if not isinstance(channel, RoomChannel):
            raise TypeError("channel must be a lipasr.room.RoomChannel")
        if channel.count > base.batch_limit:
            raise ValueError(f"a bank of {channel.count} rooms does not fit the base's batch_limit {base.batch_limit}")
        if channel.device != base.extractor.device:
            raise ValueError(f"the channel is on {channel.device}, the base on {base.extractor.device}")
        _Estimator.__init__(self, base.model, base.nb_classes)
        self.base, self.channel = base, channel
        self.utterance_length, self.domain, self.extractor = base.utterance_length, base.domain, base.extractor
        self.n, self.input_shape, self.mean, self.scale, self.clip_values = base.n, base.input_shape, base.mean, base.scale, base.clip_values
        self._bs = base.batch_limit // channel.count

    def _chunks(self, xt, lt):
        """Per chunk of batch_limit clips: (slice, the c R rows behind the channel, their lengths for the base, the channel's n_valid)."""
        r = self.channel.count
        for s in range(0, xt.shape[0], self._bs):
            sl = slice(s, s + self._bs)
            lb = None if lt is None else lt[sl]
            nv = None if lb is None else self.clip_positions(lb).contiguous()
            yield sl, self.channel.apply(xt[sl], nv), None if lb is None else lb.repeat_interleave(r), nv

    def predict_each_device(self, xt, lengths=None, logits=False):
        """[B, n] -> [B, R, classes]: the base's probabilities (or logits) for every clip through every room."""
        xt = self.rows_device(xt)
        lt = self.lengths_device(lengths, xt.shape[0])
        r = self.channel.count
        return torch.cat([self.base.predict_device(rows, logits=logits, lengths=lr).view(-1, r, self.nb_classes)
                          for _, rows, lr, _ in self._chunks(xt, lt)])

    def predict_device(self, xt, logits=False, lengths=None):
        return self.predict_each_device(xt, lengths=lengths, logits=logits).mean(dim=1)

    def loss_gradient_device(self, xt, yt, out=None, lengths=None):
        """d mean_{b, j} CE(f(features(h_j * x_b)), y_b) / dx on device tensors ([B, n], one-hot [B, classes]) -> [B, n]."""
        xt = self.rows_device(xt)
        out = torch.empty_like(xt) if out is None else out
        lt = self.lengths_device(lengths, xt.shape[0])
        r = self.channel.count
        for sl, rows, lr, nv in self._chunks(xt, lt):
            g = self.base.loss_gradient_device(rows, yt[sl].repeat_interleave(r, dim=0), lengths=lr)
            self.channel.vjp(g, nv, scale=1.0, out=out[sl])
        return out

    def output_vjp_device(self, xt, vt, on_logits=False, lengths=None):
        """sum_c v[b, c] d out_c / dx for the mean output over the rooms: [B, n], [B, classes] -> [B, n]."""
        xt = self.rows_device(xt)
        out = torch.empty_like(xt)
        lt = self.lengths_device(lengths, xt.shape[0])
        r = self.channel.count
        for sl, rows, lr, nv in self._chunks(xt, lt):
            g = self.base.output_vjp_device(rows, vt[sl].repeat_interleave(r, dim=0), on_logits=on_logits, lengths=lr)
            self.channel.vjp(g, nv, scale=1.0 / r, out=out[sl])
        return out

    def jacobian_device(self, xt, on_logits=True, lengths=None):
        """d out_c / dx of the mean output over the rooms for every class: [B, n] -> a [B, classes, n] view of class-major storage.
        Per chunk ONE Jacobian of the base at the c R rows, then one pass of the channel's adjoint per class: row c carries the bits
        of ``output_vjp_device`` with the one-hot e_c."""
        xt = self.rows_device(xt)
        b_all, c = xt.shape[0], self.nb_classes
        lt = self.lengths_device(lengths, b_all)
        r = self.channel.count
        out = torch.empty(c, b_all, self.n, device=xt.device)
        for sl, rows, lr, nv in self._chunks(xt, lt):
            jf = self.base.jacobian_device(rows, on_logits=on_logits, lengths=lr).permute(1, 0, 2)  # the base's own storage: [classes][c R][n]
            for k in range(c):
                self.channel.vjp(jf[k], nv, scale=1.0 / r, out=out[k, sl])
        return out.permute(1, 0, 2)


class DefendedClassifier(WaveformClassifier):
    """A WaveformClassifier behind an input-transformation defence: every clip goes through a lipasr.defences.AudioDefence T (a chain
    of median, FIR and bit-depth stages, one launch) before the MFCC stage.  It shares the base's model, extractor, statistics,
    domain and ``clip_values`` and takes the same rows, so any attack over audio runs on it unchanged -- which makes the attack
    ADAPTIVE: it sees the defence.  FIR taps are applied to the rows as they come, so their sample rate has to be the rows' (22 050 Hz
    in domain "22k"): that is the caller's business.  ``lengths`` keep the base's meaning (samples at ``sr_in``); the defence keeps
    every clip's length and writes exactly 0 beyond it, so they hold behind it too, and the gradient stays exactly 0 beyond each clip.
        predict_device, predict, own_labels_device                  the base's at T(x)
        loss_gradient_device, output_vjp_device, jacobian_device    the base's at T(x), carried back by ``defence.vjp(x, .)``; the
                              Jacobian takes one pass of the adjoint per class on ONE forward pass of the base
    ``backward``: "chain" differentiates through the defence (the median routes to the element it selected, the FIR is its adjoint,
    the quantiser is straight-through where its clamp was idle); "identity" takes the whole defence as the identity on the way back
    (BPDA, Athalye, Carlini and Wagner 2018): the base's gradient at T(x), masked to the clip.
    ``batch_limit`` is the base's.  A DefendedClassifier may be the base of an OverTheAirClassifier: room, then defence, then
    recogniser, the physical order."""

    def __init__(self, base, defence, backward="chain"):
        from .defences import AudioDefence

        if not isinstance(base, WaveformClassifier) or isinstance(base, (OverTheAirClassifier, DefendedClassifier)):
            raise TypeError("base must be a WaveformClassifier (and neither an OverTheAirClassifier nor a DefendedClassifier)")
        if not isinstance(defence, AudioDefence):
            raise TypeError("defence must be a lipasr.defences.AudioDefence")
        if backward not in ("chain", "identity"):
            raise ValueError(f"backward={backward!r}: 'chain' or 'identity'")
        if defence.device != base.extractor.device:
            raise ValueError(f"the defence is on {defence.device}, the base on {base.extractor.device}")
        _Estimator.__init__(self, base.model, base.nb_classes)
        self.base, self.defence, self.backward = base, defence, backward
        self.utterance_length, self.domain, self.extractor = base.utterance_length, base.domain, base.extractor
        self.n, self.input_shape, self.mean, self.scale, self.clip_values = base.n, base.input_shape, base.mean, base.scale, base.clip_values
        self._bs = base.batch_limit

    def _n_valid(self, lt):
        return None if lt is None else self.clip_positions(lt).contiguous()

    def _features(self, xb, lb):
        return self.base._features(self.defence.apply(xb.contiguous(), self._n_valid(lb)), lb)

    def features_device(self, xt, lengths=None):
        """[B <= batch_max, n] device tensor -> the standardised features of T(x)."""
        lt = self.lengths_device(lengths, xt.shape[0])
        return self._features(xt, lt)

    def predict_device(self, xt, logits=False, lengths=None):
        xt = self.rows_device(xt)
        lt = self.lengths_device(lengths, xt.shape[0])
        return self.base.predict_device(self.defence.apply(xt, self._n_valid(lt)), logits=logits, lengths=lt)

    def loss_gradient_device(self, xt, yt, out=None, lengths=None):
        """d mean CE(f(features(T(x))), y) / dx on device tensors ([B, n], one-hot [B, classes]) -> [B, n]."""
        xt = self.rows_device(xt)
        lt = self.lengths_device(lengths, xt.shape[0])
        nv = self._n_valid(lt)
        g = self.base.loss_gradient_device(self.defence.apply(xt, nv), yt, lengths=lt)
        return self.defence.vjp(xt, g, nv, backward=self.backward, out=out)

    def output_vjp_device(self, xt, vt, on_logits=False, lengths=None):
        """sum_c v[b, c] d out_c / dx with the defence in front: [B, n], [B, classes] -> [B, n]."""
        xt = self.rows_device(xt)
        lt = self.lengths_device(lengths, xt.shape[0])
        nv = self._n_valid(lt)
        g = self.base.output_vjp_device(self.defence.apply(xt, nv), vt, on_logits=on_logits, lengths=lt)
        return self.defence.vjp(xt, g, nv, backward=self.backward)

    def jacobian_device(self, xt, on_logits=True, lengths=None):
        """d out_c / dx for every class with the defence in front: [B, n] -> a [B, classes, n] view of class-major storage.  ONE
        Jacobian of the base at T(x), then one pass of the defence's adjoint per class: row c carries the bits of
        ``output_vjp_device`` with the one-hot e_c."""
        xt = self.rows_device(xt)
        b_all, c = xt.shape[0], self.nb_classes
        lt = self.lengths_device(lengths, b_all)
        nv = self._n_valid(lt)
        jf = self.base.jacobian_device(self.defence.apply(xt, nv), on_logits=on_logits, lengths=lt).permute(1, 0, 2)  # the base's own storage: [classes][B][n]
        out = torch.empty(c, b_all, self.n, device=xt.device)
        for k in range(c):
            self.defence.vjp(xt, jf[k], nv, backward=self.backward, out=out[k])
        return out.permute(1, 0, 2)
