"""attacks.py surface of the reference (attacks.py:48-86, 145-294, 496-536, 647-693) over liblipasr.

White-box: ``TensorFlowV2Classifier`` / ``FastGradientMethod`` / ``ProjectedGradientDescent`` keep
the ART constructor keywords the reference uses (``estimator=``, ``eps=``) plus the ART defaults it
relies on (norm=inf, eps_step=0.1, max_iter=100, batch_size=32, untargeted, y=None -> the model's own
predictions, no clip_values).  Each PGD iteration is ONE native call: inference forward, CE gradient,
backward to the input and the sign step fused into the last backward GEMM's epilogue (K4).  ART's other
``norm`` (1, 2), ``targeted`` and ``num_random_init`` keywords run the same call in its Lp form
(lipasr_mlp_attack_step_lp: the step is a second launch) and a native random start (lipasr_lp_ball_init).
``AutoProjectedGradientDescent`` (ART's name; Croce & Hein 2020) is PGD whose step size every row halves for itself, with the
cross-entropy or the DLR loss: per iteration the estimator's forward and backward pass and two launches of ours (lipasr/apgd.py).
The estimators live in lipasr/estimators.py (re-exported here under the same names); an attack asks its estimator for everything
that depends on what the rows are -- shape, lengths, predictions, own labels, gradients.  The one choice made here is FGM / PGD's:
over rows of features they run the fused native iteration, over audio the estimator's gradient and a step launch.
``WaveformClassifier`` puts the MFCC stage in front of the model: the same two attacks then perturb the AUDIO (eps in
amplitude units), the gradient reaching the samples through the native backward pass of K1 (lipasr_mfcc_plan_vjp).  With
``lengths=`` a batch holds clips of different lengths, one per row (lipasr_mfcc_plan_vjp_ragged): the perturbation stays inside
each clip and the rest of the row comes back untouched.  Over a short-window extractor (Speaker recognition: n_fft = win_length =
441, hop 220) the gradient goes through lipasr_mfcc_plan_vjp_short.
``OverTheAirClassifier`` puts a bank of room impulse responses (lipasr/room.py) in front of a WaveformClassifier and answers with
the expectation over the rooms: every attack over audio, white-box or black-box, then optimises the example that is PLAYED.
``DefendedClassifier`` puts an input-transformation defence (lipasr/defences.py: median, FIR and bit-depth stages) in front of a
WaveformClassifier: every attack over audio then differentiates through the defence, or takes it as the identity on the way back.

Black-box: ``standardize_dataset`` (A2, fp64-accumulated fit on the device), the audio-domain noise
models on the device (Philox RNG) and the noisy-audio -> MFCC dataset helpers.  ``GeneticAttack`` (lipasr/genetic.py,
ours) and ``SquareAttack`` (lipasr/square.py; ART's name, Andriushchenko et al. 2020) are the black-box attacks that look at the
model's answer: a genetic algorithm with pop_size score queries per generation, and a random search with one per iteration.
``HopSkipJump`` (lipasr/hopskipjump.py; ART's name, Chen et al. 2020) sees less still, the label alone, and minimises the L2 or
L-inf distance to the nearest misclassified point it can find.
``AutoAttack`` (ART's name) runs Auto-PGD with both losses, DeepFool and SquareAttack in turn over the rows that are still
classified correctly and reports the accuracy that survives all of them.
``UniversalPerturbation`` (lipasr/universal.py; ART's name, Moosavi-Dezfooli et al. 2017) fits ONE noise vector for every row --
the only attack here whose kernels sum across the rows of a batch -- and applies it to rows it never saw.
``TimeWarp`` (lipasr/warp.py; ours, ART's ``SpatialTransformation`` is the closest name) is the one threat model here that is not
additive: the worst of a grid of small delays, speeds and levels per clip, then first-order steps on the three parameters.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N
from ._rows import check_estimator, clip_pair, generate_host, labels_device, resolve_clip_values
from .estimators import DefendedClassifier, OverTheAirClassifier, TensorFlowV2Classifier, WaveformClassifier, _as_given, _dev, _Estimator, _to_dev
from .extract_features_construct_dataset import read_wav, _extractor
from .genetic import GeneticAttack  # noqa: F401  (the genetic black-box attack: scores only; lipasr/genetic.py)
from .keras import to_categorical
from .square import SquareAttack  # noqa: F401  (Square Attack: one score query per iteration; lipasr/square.py)
from .hopskipjump import HopSkipJump  # noqa: F401  (HopSkipJump: decisions only, minimum L2 / L-inf norm; lipasr/hopskipjump.py)
from .universal import UniversalPerturbation  # noqa: F401  (one noise vector for every row; lipasr/universal.py)
from .warp import TimeWarp  # noqa: F401  (worst-case shift, speed and gain over audio; lipasr/warp.py)


# ------------------------------------------------------------------------------------------------ A2
class StandardScaler:
    """sklearn.preprocessing.StandardScaler restricted to fit / transform / fit_transform, on the device.
    Statistics are fp64 (mean_, scale_ are float64 device tensors, as sklearn's are float64 arrays)."""

    def fit(self, x):
        xt = _to_dev(x)
        h = N.get_handle(xt.device.index)
        self.mean_ = torch.zeros(xt.shape[1], dtype=torch.float64, device=xt.device)
        self.scale_ = torch.zeros(xt.shape[1], dtype=torch.float64, device=xt.device)
        N.check(N.lib.lipasr_scaler_fit(h.h, N.ptr(xt), xt.shape[0], xt.shape[1], N.ptr(self.mean_), N.ptr(self.scale_), N.stream_ptr()))
        return self

    def transform_device(self, xt):
        h = N.get_handle(xt.device.index)
        out = torch.empty_like(xt)
        N.check(N.lib.lipasr_scaler_apply(h.h, N.ptr(xt), xt.shape[0], xt.shape[1], N.ptr(self.mean_), N.ptr(self.scale_), N.ptr(out), N.stream_ptr()))
        return out

    def transform(self, x):
        out = self.transform_device(_to_dev(x))
        return out if torch.is_tensor(x) else out.cpu().numpy()

    def fit_transform(self, x):
        return self.fit(x).transform(x)


def standardize_dataset(train_data, val_data, test_data):
    """attacks.py:48-69 / train_constraints.py:28-35: fit on the concatenation, split back."""
    parts = [_to_dev(train_data), _to_dev(val_data), _to_dev(test_data)]
    all_data = torch.cat(parts, dim=0)
    out = StandardScaler().fit(all_data).transform_device(all_data)
    a, b = parts[0].shape[0], parts[0].shape[0] + parts[1].shape[0]
    res = (out[:a], out[a:b], out[b:])
    if torch.is_tensor(train_data):
        return res
    return tuple(r.cpu().numpy() for r in res)


def random_targets(labels, nb_classes, rng=None):
    """ART utils.random_targets: for every sample a uniformly drawn class different from ``labels`` -> one-hot."""
    rng = np.random if rng is None else rng
    labels = np.asarray(labels)
    if labels.ndim > 1:
        labels = labels.argmax(axis=1)
    result = np.zeros(labels.shape, dtype=np.int64)
    for c in range(nb_classes):
        other = [k for k in range(nb_classes) if k != c]
        sel = labels == c
        result[sel] = rng.choice(other, size=int(sel.sum()))
    return to_categorical(result, nb_classes)


class SaliencyMapMethod:
    """ART SaliencyMapMethod(classifier=, theta=, gamma=) (JSMA; attacks.py:546-550 uses theta=10, gamma=0.1) without
    clip_values, as the reference runs it: while a sample's prediction differs from its target and at most ``gamma``
    of its features were touched, add ``theta`` to the two features with the largest target-class gradient.
    The class gradients and predictions run natively (lipasr_mlp_output_vjp / lipasr_mlp_predict).

    ``max_iter`` bounds the loop: with no clip values ART's search space never shrinks, so a sample that never
    reaches its target would loop forever there; None keeps ART's behaviour."""

    def __init__(self, classifier, theta=0.1, gamma=1.0, batch_size=1, verbose=True, max_iter=None):
        if not isinstance(classifier, TensorFlowV2Classifier):
            raise TypeError("classifier must be a lipasr TensorFlowV2Classifier")
        if not 0 < gamma <= 1:
            raise ValueError("The total perturbation percentage `gamma` must be between 0 and 1.")
        if batch_size <= 0:
            raise ValueError("The batch size `batch_size` has to be positive.")
        self.estimator, self.theta, self.gamma = classifier, float(theta), float(gamma)
        self.batch_size, self.max_iter = int(batch_size), max_iter

    def generate(self, x, y=None, rng=None):
        est = self.estimator
        m = est.model
        xt = _to_dev(x)
        adv = xt.clone()
        nf = adv.shape[1]
        preds = m.predict_device(xt).argmax(dim=1)
        if y is None:
            targets = torch.as_tensor(random_targets(preds.cpu().numpy(), est.nb_classes, rng).argmax(axis=1), device=xt.device)
        else:
            targets = torch.as_tensor(np.asarray(y.cpu() if torch.is_tensor(y) else y).argmax(axis=1), device=xt.device)
        bs = min(self.batch_size, m._max_batch)
        for s0 in range(0, adv.shape[0], bs):
            batch = adv[s0:s0 + bs]
            tgt = targets[s0:s0 + bs]
            active = torch.nonzero(preds[s0:s0 + bs] != tgt)[:, 0]
            all_feat = torch.zeros_like(batch)
            it = 0
            while active.numel() != 0 and (self.max_iter is None or it < self.max_iter):
                v = torch.zeros(active.numel(), est.nb_classes, device=xt.device)
                v[torch.arange(active.numel(), device=xt.device), tgt[active]] = 1.0
                g = est.output_vjp_device(batch[active].contiguous(), v)
                ind = torch.topk(g if self.theta > 0 else -g, 2, dim=1).indices
                rows = active[:, None].expand(-1, 2)
                all_feat[rows, ind] = 1.0
                batch[rows, ind] += self.theta
                cur = m.predict_device(batch.contiguous()).argmax(dim=1)
                active = torch.nonzero((cur != tgt) & (all_feat.sum(dim=1) / nf <= self.gamma))[:, 0]
                it += 1
        return _as_given(adv, x)


_TANH_SMOOTHER = 0.999999
_C_UPPER_BOUND = 10e10


def _to_tanh(x, lo, hi):
    return torch.atanh((torch.minimum(torch.maximum(x, lo), hi) - lo) / (hi - lo) * (2 * _TANH_SMOOTHER) - _TANH_SMOOTHER)


def _from_tanh(xt, lo, hi):
    return (torch.tanh(xt) / _TANH_SMOOTHER + 1.0) / 2.0 * (hi - lo) + lo


class _Carlini:
    """Shared pieces of ART's Carlini & Wagner attacks as the reference calls them (attacks.py:571-645): untargeted,
    y=None (labels := the estimator's own predictions), no clip_values.  ART evaluates the margin on the model
    OUTPUT -- softmax probabilities for this Keras model -- so with the reference's confidence >= 1 the success test
    can never hold; that behaviour is kept.  Predictions and the class-gradient difference run natively
    (lipasr_mlp_predict, lipasr_mlp_output_vjp); the line-search bookkeeping is a handful of elementwise tensor
    ops per iteration.  Restated from ART 1.9-1.10's published implementation (ART is absent: parity unpinned)."""

    def __init__(self, classifier, confidence, targeted, learning_rate, max_iter, max_halving, max_doubling, batch_size):
        if not isinstance(classifier, TensorFlowV2Classifier):
            raise TypeError("classifier must be a lipasr TensorFlowV2Classifier")
        if targeted:
            raise NotImplementedError("the reference runs the untargeted attack")
        if max_iter < 0 or max_halving < 1 or max_doubling < 1 or batch_size < 1:
            raise ValueError("max_iter >= 0, max_halving >= 1, max_doubling >= 1 and batch_size >= 1 are required")
        self.estimator, self.confidence, self.learning_rate = classifier, float(confidence), float(learning_rate)
        self.max_iter, self.max_halving, self.max_doubling, self.batch_size = int(max_iter), int(max_halving), int(max_doubling), int(batch_size)

    def _predict(self, xa):
        return self.estimator.model.predict_device(xa.contiguous())

    def _margin(self, z, target):
        z_target = (z * target).sum(dim=1)
        z_other = (z * (1 - target) + (z.min(dim=1).values - 1)[:, None] * target).max(dim=1).values
        return torch.clamp(z_target - z_other + self.confidence, min=0.0)

    def _grad_diff(self, z, target, xa):
        other = (z * (1 - target) + (z.min(dim=1).values - 1)[:, None] * target).argmax(dim=1)
        v = target.clone()                                   # +1 at the label (i_add) ...
        v[torch.arange(z.shape[0], device=z.device), other] -= 1.0   # ... -1 at the best other class (i_sub)
        return self.estimator.output_vjp_device(xa.contiguous(), v)

    def _labels(self, xt, y):
        return _to_dev(y) if y is not None else self.estimator.own_labels_device(xt)

    def _line_search(self, n, active, loss, pert, lr, evaluate):
        """ART's halving / doubling search on the per-sample learning rate; evaluate(sel, step) -> loss of the trial
        points x_tanh[sel] + step * pert_rows.  Returns best_lr (0 where no trial improved the loss)."""
        prev_loss, best_loss = loss.clone(), loss.clone()
        best_lr = torch.zeros(n, device=loss.device)
        halving = torch.zeros(n, device=loss.device)
        idx = torch.nonzero(active)[:, 0]
        for _ in range(self.max_halving):
            do = loss[idx] >= prev_loss[idx]
            if not bool(do.any()):
                break
            sel = idx[do]
            loss[sel] = evaluate(sel, lr[sel], pert[do])
            better = loss < best_loss
            best_lr[better] = lr[better]
            best_loss[better] = loss[better]
            lr[sel] /= 2
            halving[sel] += 1
        lr[idx] *= 2
        for _ in range(self.max_doubling):
            do = (halving[idx] == 1) & (loss[idx] <= best_loss[idx])
            if not bool(do.any()):
                break
            sel = idx[do]
            lr[sel] *= 2
            loss[sel] = evaluate(sel, lr[sel], pert[do])
            better = loss < best_loss
            best_lr[better] = lr[better]
            best_loss[better] = loss[better]
        lr[halving == 1] /= 2
        return best_lr


class CarliniL2Method(_Carlini):
    """ART CarliniL2Method(classifier=, confidence=) (attacks.py:606-616: confidence in linspace(1, 300, 3))."""

    def __init__(self, classifier, confidence=0.0, targeted=False, learning_rate=0.01, binary_search_steps=10, max_iter=10,
                 initial_const=0.01, max_halving=5, max_doubling=5, batch_size=1, verbose=True):
        super().__init__(classifier, confidence, targeted, learning_rate, max_iter, max_halving, max_doubling, batch_size)
        self.binary_search_steps, self.initial_const = int(binary_search_steps), float(initial_const)

    def generate(self, x, y=None):
        xt = _to_dev(x)
        adv = xt.clone()
        lo = torch.tensor(float(xt.min()), device=xt.device)
        hi = torch.tensor(float(xt.max()), device=xt.device)
        yt = self._labels(xt, y)
        bs = min(self.batch_size, self.estimator.model._max_batch)
        for s0 in range(0, xt.shape[0], bs):
            xb, yb = xt[s0:s0 + bs], yt[s0:s0 + bs]
            n = xb.shape[0]
            xb_tanh = _to_tanh(xb, lo, hi)
            c_cur = torch.full((n,), self.initial_const, device=xt.device)
            c_lower = torch.zeros(n, device=xt.device)
            c_double = torch.ones(n, dtype=torch.bool, device=xt.device)
            best_l2 = torch.full((n,), float("inf"), device=xt.device)
            best_adv = xb.clone()

            def loss_fn(sel, xa_sel):
                l2 = ((xb[sel] - xa_sel) ** 2).sum(dim=1)
                z = self._predict(xa_sel)
                return z, l2, c_cur[sel] * self._margin(z, yb[sel]) + l2

            everyone = torch.arange(n, device=xt.device)
            for _bss in range(self.binary_search_steps):
                if not bool((c_cur < _C_UPPER_BOUND).any()):
                    break
                lr = torch.full((n,), self.learning_rate, device=xt.device)
                xa, xa_tanh = xb.clone(), xb_tanh.clone()
                z, l2, loss = loss_fn(everyone, xa)
                success = loss - l2 <= 0
                overall = success.clone()
                for _it in range(self.max_iter):
                    improved = success & (l2 < best_l2)
                    best_l2[improved] = l2[improved]
                    best_adv[improved] = xa[improved]
                    active = (c_cur < _C_UPPER_BOUND) & (lr > 0)
                    if not bool(active.any()):
                        break
                    g = self._grad_diff(z[active], yb[active], xa[active])
                    g = g * c_cur[active][:, None] + 2 * (xa[active] - xb[active])
                    g = g * (hi - lo) * (1 - torch.tanh(xa_tanh[active]) ** 2) / (2 * _TANH_SMOOTHER)
                    pert = -g

                    def evaluate(sel, step, rows):
                        new_x = _from_tanh(xa_tanh[sel] + step[:, None] * rows, lo, hi)
                        _, l2[sel], ls = loss_fn(sel, new_x)
                        return ls

                    best_lr = self._line_search(n, active, loss, pert, lr, evaluate)
                    idx = torch.nonzero(active)[:, 0]
                    upd = best_lr[idx] > 0
                    if bool(upd.any()):
                        sel = idx[upd]
                        xa_tanh[sel] = xa_tanh[sel] + best_lr[sel][:, None] * pert[upd]
                        xa[sel] = _from_tanh(xa_tanh[sel], lo, hi)
                        z[sel], l2[sel], loss[sel] = loss_fn(sel, xa[sel])
                        success = loss - l2 <= 0
                        overall = overall | success
                improved = success & (l2 < best_l2)
                best_l2[improved] = l2[improved]
                best_adv[improved] = xa[improved]
                c_double[overall] = False
                c_old = c_cur.clone()
                c_cur[overall] = c_lower[overall] + (c_cur - c_lower)[overall] / 2
                fail = ~overall
                c_lower[fail] = c_old[fail]
                fd = fail & c_double
                c_cur[fd] = c_cur[fd] * 2
                nd = fail & ~c_double
                c_cur[nd] = c_cur[nd] + (c_cur - c_lower)[nd] / 2
            adv[s0:s0 + bs] = best_adv
        return _as_given(adv, x)


class CarliniLInfMethod(_Carlini):
    """ART CarliniLInfMethod(classifier=, confidence=) (attacks.py:578-582: confidence = 10), eps = 0.3."""

    def __init__(self, classifier, confidence=0.0, targeted=False, learning_rate=0.01, max_iter=10, max_halving=5, max_doubling=5,
                 eps=0.3, batch_size=128, verbose=True):
        super().__init__(classifier, confidence, targeted, learning_rate, max_iter, max_halving, max_doubling, batch_size)
        if eps <= 0:
            raise ValueError("The eps parameter must be strictly positive.")
        self.eps = float(eps)

    def generate(self, x, y=None):
        xt = _to_dev(x)
        adv = xt.clone()
        yt = self._labels(xt, y)
        bs = min(self.batch_size, self.estimator.model._max_batch)
        for s0 in range(0, xt.shape[0], bs):
            xb, yb = xt[s0:s0 + bs], yt[s0:s0 + bs]
            n = xb.shape[0]
            lo, hi = xb - self.eps, xb + self.eps
            xa, xa_tanh = xb.clone(), _to_tanh(xb, lo, hi)
            z = self._predict(xa)
            loss = self._margin(z, yb)
            lr = torch.full((n,), self.learning_rate, device=xt.device)
            for _it in range(self.max_iter):
                active = (loss > 0) & (lr > 0)
                if not bool(active.any()):
                    break
                g = self._grad_diff(z[active], yb[active], xa[active])
                pert = -(g * (hi - lo)[active] * (1 - torch.tanh(xa_tanh[active]) ** 2) / (2 * _TANH_SMOOTHER))

                def evaluate(sel, step, rows):
                    new_x = _from_tanh(xa_tanh[sel] + step[:, None] * rows, lo[sel], hi[sel])
                    return self._margin(self._predict(new_x), yb[sel])

                best_lr = self._line_search(n, active, loss, pert, lr, evaluate)
                idx = torch.nonzero(active)[:, 0]
                upd = best_lr[idx] > 0
                if bool(upd.any()):
                    sel = idx[upd]
                    xa_tanh[sel] = xa_tanh[sel] + best_lr[sel][:, None] * pert[upd]
                    xa[sel] = _from_tanh(xa_tanh[sel], lo[sel], hi[sel])
                z = self._predict(xa)
                loss = self._margin(z, yb)
            adv[s0:s0 + bs] = xa
        return _as_given(adv, x)


_NORMS = {np.inf: math.inf, "inf": math.inf, 1: 1.0, 2: 2.0}
_ball_calls = [0]


def _norm_value(norm):
    """ART's norm keyword (np.inf, "inf", 1, 2) -> the float the C ABI takes (inf, 1.0, 2.0)."""
    try:
        return _NORMS[norm]
    except (KeyError, TypeError):
        raise ValueError(f"norm={norm!r}: np.inf, 'inf', 1 and 2 are supported") from None


class _SignAttack:
    """FGM / PGD over the native iteration.  norm=inf, untargeted, no random start (the reference's call) runs
    lipasr_mlp_attack_step, whose K4 sign step is fused into the last backward GEMM; every other setting runs
    lipasr_mlp_attack_step_lp (norm inf: the same fused launch; norm 1, 2: dX GEMM + the row-wise Lp step kernel).
    ART semantics (1.9-1.10, restated -- parity unpinned): targeted=True descends the CE toward ``y`` (required); with
    num_random_init = k > 0 every one of the max(1, k) restarts starts from x0 + a draw of ART's random_sphere
    (lipasr_lp_ball_init) before its first iteration."""

    def __init__(self, estimator, eps, eps_step, max_iter, batch_size, norm, targeted, num_random_init):
        if not isinstance(estimator, (TensorFlowV2Classifier, WaveformClassifier)):
            raise TypeError("estimator must be a lipasr TensorFlowV2Classifier or WaveformClassifier")
        # the rows are the model's own inputs: the fused native iteration applies (the one choice this class makes by estimator)
        self._fused = isinstance(estimator, TensorFlowV2Classifier)
        self.norm = _norm_value(norm)
        if int(num_random_init) < 0:
            raise ValueError("num_random_init must be >= 0")
        self.estimator, self.eps, self.eps_step = estimator, float(eps), float(eps_step)
        self._default_eps = self.eps  # the ball of the reference's call (FastGradientMethod: none)
        self.max_iter, self.batch_size = int(max_iter), int(batch_size)
        self.targeted, self.num_random_init = bool(targeted), int(num_random_init)
        # random starts: Philox key (seed, restart, first row of the batch) and a device counter that moves with every generate()
        _ball_calls[0] += 1
        self.seed = 0xBA11000000000000 + _ball_calls[0]
        self._draws = None

    @property
    def _default_path(self):
        return math.isinf(self.norm) and not self.targeted and self.num_random_init == 0

    def _step(self, xa, x0, yb):
        """One native iteration over rows of features, in place on xa."""
        m = self.estimator.model
        if self._default_path:
            N.check(N.lib.lipasr_mlp_attack_step(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xa), N.ptr(x0), N.ptr(yb), xa.shape[0],
                                                 self.eps_step, self._default_eps, N.stream_ptr()))
        else:
            a = -self.eps_step if self.targeted else self.eps_step  # ART: gradient x (1 - 2 targeted)
            N.check(N.lib.lipasr_mlp_attack_step_lp(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xa), N.ptr(x0), N.ptr(yb),
                                                    xa.shape[0], self.norm, a, self.eps, N.stream_ptr()))

    def _random_init(self, xa, x0, restart, row0):
        """xa <- x0 + one draw of ART's random_sphere(rows, n, eps, norm) for restart ``restart`` of the rows starting at
        ``row0`` of the generate() call (the Philox key: (seed, restart, row0); the counter: this attack's generate() count)."""
        key = (self.seed + 0x9E3779B97F4A7C15 * (restart + 1) + 0xBF58476D1CE4E5B9 * row0) & 0xFFFFFFFFFFFFFFFF
        h = N.get_handle(xa.device.index)
        N.check(N.lib.lipasr_lp_ball_init(h.h, N.ptr(xa), N.ptr(x0), xa.shape[0], xa.shape[1], self.norm, self.eps, key,
                                          N.ptr(self._draws), 0, N.stream_ptr()))

    def _start(self, xa, x0, restart, row0):
        if self.num_random_init > 0:
            self._random_init(xa, x0, restart, row0)
        else:
            xa.copy_(x0)

    def _success(self, est, x0, yb, xa, lens):
        """ART compute_success_array: argmax at xa == target (targeted) or != the clean prediction (untargeted).  The rows are
        whole row slices of contiguous tensors, as the estimator takes them."""
        pa = est.predict_device(xa, logits=True, lengths=lens).argmax(dim=1)
        if self.targeted:
            return pa == yb.argmax(dim=1)
        return pa != est.predict_device(x0, logits=True, lengths=lens).argmax(dim=1)

    # ---- over audio (WaveformClassifier): features -> lipasr_mlp_input_grad -> MFCC backward -> lipasr_lp_step -> clamp, all on
    # the device; every keyword keeps its meaning, eps and eps_step are amplitudes
    # With per-clip lengths (lens: int32 [rows], mask: bool [rows, n], the positions inside each clip) the iterate lives inside the
    # clip: the gradient is exactly 0 outside it, a random start is multiplied by the mask (the draw only shrinks: it stays in the
    # eps ball for norms 1 and 2 as well), and after every clamp the rest of the row is put back from x0 bit for bit (clip_values
    # is not applied there).
    def _wave_clamp(self, est, xa, x0, mask):
        if mask is None:
            if est.clip_values is not None:
                xa.clamp_(*est.clip_values)
            return
        inside = xa if est.clip_values is None else xa.clamp(*est.clip_values)
        xa.copy_(torch.where(mask, inside, x0))

    def _wave_attack_rows(self, est, xa, x0, yb, restart, row0, g, lens=None, mask=None):
        h = N.get_handle(xa.device.index)
        self._start(xa, x0, restart, row0)
        if self.num_random_init > 0:
            self._wave_clamp(est, xa, x0, mask)
        alpha = -self.eps_step if self.targeted else self.eps_step
        for _ in range(self.max_iter):
            est.loss_gradient_device(xa, yb, out=g, lengths=lens)
            N.check(N.lib.lipasr_lp_step(h.h, N.ptr(xa), N.ptr(x0), N.ptr(g), xa.shape[0], xa.shape[1], self.norm, alpha, self.eps,
                                         N.stream_ptr()))
            self._wave_clamp(est, xa, x0, mask)

    # ---- the restart driver.  The row backend is batch(s) -> (attack, success) for the rows starting at s: attack(xa, restart) does
    # "start, then max_iter iterations" in place on xa, success(xa) is ART's compute_success_array on those rows.
    def _rows(self, xt, yt, lt, bs):
        est = self.estimator
        y_all = yt if yt is not None else est.own_labels_device(xt, lengths=lt, batch=bs)
        mask_all = None if lt is None else est.clip_mask(lt)
        cut = lambda t, s: None if t is None else t[s:s + bs]
        g = None if self._fused else torch.empty(bs, xt.shape[1], device=xt.device)

        def batch(s):
            x0, yb, lb = xt[s:s + bs], y_all[s:s + bs], cut(lt, s)

            def attack(xa, restart):
                if not self._fused:
                    return self._wave_attack_rows(est, xa, x0, yb, restart, s, g[:x0.shape[0]], lb, cut(mask_all, s))
                self._start(xa, x0, restart, s)
                for _ in range(self.max_iter):
                    self._step(xa, x0, yb)
            return attack, lambda xa: self._success(est, x0, yb, xa, lb)
        return batch

    def _generate_restarts(self, xt, bs, batch):
        rows = range(0, xt.shape[0], bs)
        restarts = max(1, self.num_random_init)
        adv = torch.empty_like(xt)
        if not self._best_whole_restart:  # restart 0 is kept, every later restart overwrites the rows where it succeeds
            for s in rows:
                attack, success = batch(s)
                out = adv[s:s + bs]
                xa = torch.empty_like(out)
                for r in range(restarts):
                    attack(xa, r)
                    if r == 0:
                        out.copy_(xa)
                    else:
                        ok = success(xa)
                        out[ok] = xa[ok]
            return adv
        best, best_rate = adv, None  # the whole restart with the highest success rate, the first on ties
        for r in range(restarts):
            cur = adv if r == 0 else torch.empty_like(xt)
            for s in rows:
                batch(s)[0](cur[s:s + bs], r)
            if restarts > 1:
                rate = float(torch.cat([batch(s)[1](cur[s:s + bs]) for s in rows]).float().mean())
                if best_rate is None or rate > best_rate:
                    best, best_rate = cur, rate
        return best

    def generate_device(self, xt, yt=None, lengths=None):
        """x: float32 device tensor; returns a NEW device tensor (the input is left untouched).  lengths (WaveformClassifier only):
        the samples of each row that belong to its clip, as WaveformClassifier takes them; every keyword keeps its meaning per row,
        the perturbation stays inside the clip and the rest of each row is returned as it came."""
        est = self.estimator
        lt = est.lengths_device(lengths, len(xt))  # first: rows of features take none, whatever else is wrong
        xt = est.rows_device(xt)
        if self.targeted and yt is None:
            raise ValueError("Target labels `y` need to be provided for a targeted attack.")
        bs = min(self.batch_size, est.batch_limit)
        if self._default_path and self._fused:  # the reference's call: labels, then max_iter fused launches, per batch
            adv = xt.clone()
            for s in range(0, xt.shape[0], bs):
                x0 = xt[s:s + bs]
                xa = adv[s:s + bs]
                yb = est.own_labels_device(x0, batch=bs) if yt is None else yt[s:s + bs]
                for _ in range(self.max_iter):
                    self._step(xa, x0, yb)
            return adv
        if self._draws is None:
            self._draws = torch.zeros(1, dtype=torch.int32, device=xt.device)
        adv = self._generate_restarts(xt, bs, self._rows(xt, yt, lt, bs))
        self._draws += 1  # the next generate() draws fresh random starts
        return adv

    def generate(self, x, y=None, lengths=None):
        lt = self.estimator.lengths_device(lengths, len(x))
        xt = _to_dev(x)
        yt = None if y is None else _to_dev(y)
        adv = self.generate_device(xt, yt, lt)
        return _as_given(adv, x)


class FastGradientMethod(_SignAttack):
    """ART FastGradientMethod(estimator=, eps=) (attacks.py:506-510): x + eps * d(grad), one step.  d = sign (norm inf: no
    clipping on the reference's call), g / ||g||_1 or g / ||g||_2, projected on the eps ball around x as ART does.
    num_random_init = k > 1 keeps the whole restart with the highest success rate (the first on ties: ART's compute_success)."""

    _best_whole_restart = True

    def __init__(self, estimator, eps=0.3, batch_size=32, norm=np.inf, targeted=False, num_random_init=0):
        super().__init__(estimator, eps, eps, 1, batch_size, norm, targeted, num_random_init)
        self._default_eps = math.inf  # the reference's call is one step of eps from x0: alpha = eps, and no ball to project on


class ProjectedGradientDescent(_SignAttack):
    """ART ProjectedGradientDescent(estimator=, eps=) (attacks.py:657-661): max_iter steps of
    x <- x0 + P_eps(x + eps_step * d(grad) - x0), d and P as FastGradientMethod's.  With num_random_init = k > 0, restart 0's
    result is kept and every later restart overwrites the rows where it succeeds (ART's compute_success_array)."""

    _best_whole_restart = False

    def __init__(self, estimator, eps=0.3, eps_step=0.1, max_iter=100, batch_size=32, norm=np.inf, targeted=False, num_random_init=0):
        super().__init__(estimator, eps, eps_step, max_iter, batch_size, norm, targeted, num_random_init)


class AutoProjectedGradientDescent:
    """ART AutoProjectedGradientDescent(estimator=, norm=, eps=, eps_step=, max_iter=, targeted=, nb_random_init=, batch_size=,
    loss_type=) (Croce & Hein 2020, Auto-PGD): projected gradient ascent with momentum whose step size every input halves for
    itself when its own loss stops improving, restarting from its own best point.  ``norm``: np.inf or 2 (1 is refused);
    ``eps_step``: the first step size, None: the paper's 2 eps; ``loss_type``: "cross_entropy" or "difference_logits_ratio" (the
    scale-invariant DLR loss, untargeted, at least 3 classes); ``targeted``: y holds the class to reach (required then);
    y=None: the model's own labels.  After the ``*``, ours: ``clip_values`` (default: the estimator's; a TensorFlowV2Classifier has
    none) and ``seed`` (of the random starts).

    Over a TensorFlowV2Classifier (rows of features) or a WaveformClassifier (audio, with ``lengths=`` as PGD takes them: the
    perturbation stays inside each clip and the rest of the row comes back bit for bit).  Per batch of min(batch_size,
    estimator.batch_limit) rows and restart: the start is x0 (nb_random_init == 0) or a lipasr_lp_ball_init draw keyed by (seed,
    restart, first row of the batch), clamped and masked as PGD's; then max_iter times predict_device(logits=True) -> apgd_loss ->
    output_vjp_device(on_logits=True) -> apgd_step, the checkpoints from ``apgd_checkpoints(max_iter)``; then one last forward pass
    and an apgd_step with LAST.  Two launches of ours per iteration besides the estimator's two passes; nothing returns to the host
    inside a restart.  Every one of the max(1, nb_random_init) restarts runs all rows of the batch (a draw stays a function of the
    row index); a batch whose rows are all fooled skips its remaining restarts; a fooled row keeps the first restart that fooled it,
    any other row the restart with the highest best loss.

    generate / generate_device return a NEW array: per row the most recent misclassified iterate where there is one, else the
    iterate of highest loss.  Afterwards ``success_`` (bool), ``loss_`` (float32: the best loss of the run the row's result comes
    from) and ``halvings_`` (int32: how often that run halved the row's step), device tensors [B].

    Where this differs from ART (restated from memory of its published implementation; ART is absent: parity unpinned): ART keeps
    ONE step size and one mean loss per batch; this class keeps them per row, as the paper and its authors' code do, so a row's
    result does not depend on its neighbours.  Condition 1 counts an iteration as improving when its loss exceeds the PREVIOUS
    iterate's, as the paper words it.  After a restart from the best point the momentum term is zero for one step."""

    _UNSET = object()

    def __init__(self, estimator, norm=np.inf, eps=0.3, eps_step=None, max_iter=100, targeted=False, nb_random_init=5, batch_size=32,
                 loss_type="cross_entropy", *, clip_values=_UNSET, seed=0):
        from .apgd import _loss_code, apgd_checkpoints

        check_estimator(estimator, (TensorFlowV2Classifier, WaveformClassifier))
        self.norm = _norm_value(norm)
        if self.norm == 1.0:
            raise ValueError("norm=1: Auto-PGD runs in norm 2 or np.inf")
        self.estimator, self.eps = estimator, float(eps)
        self.eps_step = 2.0 * self.eps if eps_step is None else float(eps_step)
        if not (0.0 <= self.eps < math.inf and 0.0 <= self.eps_step < math.inf):
            raise ValueError(f"eps = {eps}, eps_step = {eps_step}: finite, non-negative numbers are required")
        self.max_iter, self.batch_size, self.nb_random_init = int(max_iter), int(batch_size), int(nb_random_init)
        if self.max_iter < 1 or self.batch_size < 1 or self.nb_random_init < 0:
            raise ValueError("max_iter >= 1, batch_size >= 1 and nb_random_init >= 0 are required")
        self.targeted, self.loss_type = bool(targeted), loss_type
        self._loss = _loss_code(loss_type)
        if self._loss == 1 and self.targeted:
            raise ValueError("loss_type='difference_logits_ratio' is untargeted only")
        if self._loss == 1 and estimator.nb_classes < 3:
            raise ValueError(f"loss_type='difference_logits_ratio' needs at least 3 classes, the estimator has {estimator.nb_classes}")
        self.clip_values = resolve_clip_values(estimator, clip_values, AutoProjectedGradientDescent._UNSET)
        self.seed = (0xA9D0000000000000 + int(seed)) & 0xFFFFFFFFFFFFFFFF
        self._ckpt = {}
        prev = 0
        for w in apgd_checkpoints(self.max_iter):
            self._ckpt[w], prev = w - prev, w
        self.success_ = self.loss_ = self.halvings_ = None

    def _start(self, x, x0, restart, row0, mask):
        if self.nb_random_init == 0:
            x.copy_(x0)
            return
        key = (self.seed + 0x9E3779B97F4A7C15 * (restart + 1) + 0xBF58476D1CE4E5B9 * row0) & 0xFFFFFFFFFFFFFFFF  # as _SignAttack's
        h = N.get_handle(x.device.index)
        N.check(N.lib.lipasr_lp_ball_init(h.h, N.ptr(x), N.ptr(x0), x.shape[0], x.shape[1], self.norm, self.eps, key, None, 0,
                                          N.stream_ptr()))
        inside = x if self.clip_values is None else x.clamp(*self.clip_values)
        x.copy_(inside if mask is None else torch.where(mask, inside, x0))

    def _run(self, x0, lab, lb, mask, nv, restart, row0):
        """One restart over the rows x0 -> (x_best, x_adv, state)."""
        from .apgd import apgd_loss, apgd_state, apgd_step

        est = self.estimator
        b, dev = x0.shape[0], x0.device
        x = torch.empty_like(x0)
        self._start(x, x0, restart, row0, mask)
        x_prev, x_best, g_best, x_adv = x0.clone(), x0.clone(), torch.zeros_like(x0), x0.clone()
        f, hit = torch.empty(b, device=dev), torch.empty(b, dtype=torch.int32, device=dev)
        dz = torch.empty(b, est.nb_classes, device=dev)
        state = apgd_state(b, dev)
        kw = dict(norm=self.norm, eps=self.eps, eta0=self.eps_step, clip_values=self.clip_values, n_valid=nv)
        g = None
        for k in range(self.max_iter):
            apgd_loss(est.predict_device(x, logits=True, lengths=lb), lab, self._loss, self.targeted, f=f, dz=dz, hit=hit)
            g = est.output_vjp_device(x, dz, on_logits=True, lengths=lb)
            apgd_step(x, x_prev, x0, g, x_best, g_best, x_adv, f, hit, state, first=k == 0, ckpt_len=self._ckpt.get(k, 0), **kw)
        apgd_loss(est.predict_device(x, logits=True, lengths=lb), lab, self._loss, self.targeted, f=f, dz=dz, hit=hit)
        apgd_step(x, x_prev, x0, g, x_best, g_best, x_adv, f, hit, state, last=True, **kw)
        return x_best, x_adv, state

    def generate_device(self, xt, yt=None, lengths=None):
        """xt: float32 device tensor [B, features or samples]; yt: one-hot [B, classes], class indices [B] or None; returns a NEW
        device tensor (the input is left untouched)."""
        est = self.estimator
        lt = est.lengths_device(lengths, len(xt))
        xt = est.rows_device(xt)
        b, dev = xt.shape[0], xt.device
        bs = min(self.batch_size, int(est.batch_limit))
        lab_all = labels_device(xt, yt, self.targeted, lambda: est.own_labels_device(xt, lengths=lt, batch=bs))
        mask_all = None if lt is None else est.clip_mask(lt)
        adv = xt.clone()
        self.success_ = torch.zeros(b, dtype=torch.bool, device=dev)
        self.loss_ = torch.full((b,), -math.inf, device=dev)
        self.halvings_ = torch.zeros(b, dtype=torch.int32, device=dev)
        if b == 0 or xt.shape[1] == 0:
            return adv
        for s in range(0, b, bs):
            x0 = xt[s:s + bs]
            lb = None if lt is None else lt[s:s + bs]
            mask = None if mask_all is None else mask_all[s:s + bs]
            nv = None if mask is None else mask.sum(dim=1).to(torch.int32).contiguous()
            done = torch.zeros(x0.shape[0], dtype=torch.bool, device=dev)
            for r in range(max(1, self.nb_random_init)):
                if r > 0 and bool(done.all()):
                    break
                x_best, x_adv, st = self._run(x0, lab_all[s:s + bs], lb, mask, nv, r, s)
                fooled = st["fooled"] != 0
                take = fooled | (st["f_best"] > self.loss_[s:s + bs]) if r > 0 else torch.ones_like(done)
                take = take & ~done
                adv[s:s + bs] = torch.where(take[:, None], torch.where(fooled[:, None], x_adv, x_best), adv[s:s + bs])
                self.loss_[s:s + bs] = torch.where(take, st["f_best"], self.loss_[s:s + bs])
                self.halvings_[s:s + bs] = torch.where(take, st["halvings"], self.halvings_[s:s + bs])
                done = done | fooled
            self.success_[s:s + bs] = done
        return adv

    def generate(self, x, y=None, lengths=None):
        return generate_host(self, x, y, lengths)


def deepfool_step(jac, out, label, x, norm=2, overshoot=0.02, clip_values=None, allowed=None):
    """One DeepFool iteration in place on ``x`` (lipasr_deepfool_step; include/lipasr.h fixes the conventions).  Device tensors:
    jac float32 [B, classes, n] (any strides along the first two dimensions), out float32 [B, classes], label int32 [B],
    x float32 [B, n] contiguous, allowed int32 [B] (bit k: class k may be the target) or None.
    -> (dist float32 [B], target int32 [B], state int32 [B]: 1 stepped, 0 already flipped, -1 not finite)."""
    if not (torch.is_tensor(jac) and jac.is_cuda and jac.dtype == torch.float32 and jac.dim() == 3):
        raise ValueError("jac must be a float32 device tensor [B, classes, n]")
    b, c, n = jac.shape
    if n > 1 and jac.stride(2) != 1:
        raise ValueError("jac must be contiguous along its last dimension")
    if tuple(x.shape) != (b, n) or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"x must be a contiguous float32 tensor [{b}, {n}]")
    if tuple(out.shape) != (b, c) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor [{b}, {c}]")
    if tuple(label.shape) != (b,) or label.dtype != torch.int32 or (allowed is not None and (tuple(allowed.shape) != (b,) or allowed.dtype != torch.int32)):
        raise ValueError(f"label (and allowed) must be int32 tensors [{b}]")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x.device.index)
    dist = torch.empty(b, device=x.device)
    target = torch.empty(b, dtype=torch.int32, device=x.device)
    state = torch.empty(b, dtype=torch.int32, device=x.device)
    N.check(N.lib.lipasr_deepfool_step(h.h, N.ptr(jac), jac.stride(0), jac.stride(1), N.ptr(out), N.ptr(label), N.ptr(allowed), b, c, n,
                                       _norm_value(norm), float(overshoot), lo, hi, N.ptr(x), N.ptr(dist), N.ptr(target), N.ptr(state),
                                       N.stream_ptr()))
    return dist, target, state


class DeepFool:
    """ART DeepFool(classifier=, max_iter=, epsilon=, nb_grads=, batch_size=, verbose=) (Moosavi-Dezfooli et al. 2016): the
    minimal-perturbation attack.  The positional and ART keywords mean what they mean in ART, restated from memory of its published
    implementation (ART is absent: parity unpinned): labels are the estimator's own argmax at ``x``; every iteration moves each row
    that is still in its class onto the nearest boundary of the classifier linearised at the row; the loop ends when every row has
    left its class or after ``max_iter`` iterations; ``epsilon`` is the final overshoot, x_adv = x + (1 + epsilon) (x_iter - x),
    then clipping.  One iteration is: the estimator's outputs, its Jacobian (``jacobian_device``: every class gradient from one
    forward pass) and ONE lipasr_deepfool_step for the batch; the host looks at the state vector every CHECK_EVERY iterations
    only, so nothing synchronises per iteration (a row that has left its class is left alone by the kernel).

    Ours, after the ``*``:
    ``overshoot``: the paper's per-step overshoot, x <- x + (1 + overshoot) r.  ART has none (``overshoot=0`` is its iteration):
    its step lands exactly ON the boundary of a piecewise-linear network, where the argmax is decided by rounding, and such rows
    then take zero-length steps until max_iter.  With 0.02 they leave.
    ``norm``: 2 (ART's) or np.inf (the paper's l_p form with p = inf: the step is |f| / ||w||_1 sign(w)).
    ``on_logits``: True differentiates the logits, for which the linearisation is exact inside a ReLU piece; False the softmax
    probabilities, what ART does with a Keras model that ends in softmax (and warns about).
    ``nb_grads`` < nb_classes: the candidates of a ROW are its own nb_grads largest outputs at x.  ART takes the union of those
    classes over the whole array, so a row's result there depends on its neighbours; here it does not.

    Estimators: TensorFlowV2Classifier (rows of features, no clipping) and WaveformClassifier in either domain, with ``lengths=``
    and over a short-window extractor; over audio the kernel clamps to the classifier's ``clip_values``, and with ``lengths=`` the
    rest of each row comes back as it was.  Rows go through in chunks bounded by the estimator's ``batch_limit`` and by
    JACOBIAN_CHUNK_BYTES for one chunk's Jacobian; ``batch_size`` is accepted and ignored above that.
    After a call ``self.last`` holds NumPy arrays [B]: ``iterations`` (steps taken), ``flipped`` (from a final prediction on
    x_adv), ``target`` (the class of the last step's boundary, -1 without a step) and ``first_dist`` (rho_l of the first step: the
    distance to the linearised boundary at x)."""

    CHECK_EVERY = 4

    def __init__(self, classifier, max_iter=100, epsilon=1e-6, nb_grads=10, batch_size=1, verbose=True, *, norm=2, overshoot=0.02,
                 on_logits=True):
        if not isinstance(classifier, _Estimator):
            raise TypeError("classifier must be a lipasr TensorFlowV2Classifier or WaveformClassifier")
        if int(max_iter) < 0 or int(nb_grads) < 1 or int(batch_size) < 1:
            raise ValueError("max_iter >= 0, nb_grads >= 1 and batch_size >= 1 are required")
        if float(epsilon) < 0 or not (0 <= float(overshoot) < math.inf):
            raise ValueError("epsilon and overshoot must not be negative")
        self.norm = _norm_value(norm)
        if self.norm == 1.0:
            raise ValueError("norm=1: DeepFool runs in norm 2 or np.inf")
        if classifier.nb_classes > 32:
            raise ValueError(f"{classifier.nb_classes} classes; 1 to 32 are supported")
        self.estimator = classifier
        self.max_iter, self.epsilon, self.nb_grads, self.batch_size = int(max_iter), float(epsilon), int(nb_grads), int(batch_size)
        self.overshoot, self.on_logits, self.verbose = float(overshoot), bool(on_logits), verbose
        self.last = None

    def _chunk(self, x0, lt):
        """The rows ``x0`` (one chunk) -> (x_adv, iterations, flipped, target, first_dist) on the device."""
        est = self.estimator
        b, c = x0.shape[0], est.nb_classes
        clip = est.clip_values
        out0 = est.predict_device(x0, logits=self.on_logits, lengths=lt)
        classes = torch.arange(c, device=x0.device, dtype=torch.int32)
        label = torch.where(out0 == out0.max(dim=1, keepdim=True).values, classes[None, :], c).min(dim=1).values.to(torch.int32)
        allowed = None
        if self.nb_grads < c:
            bits = (torch.ones(1, dtype=torch.int64, device=x0.device) << torch.topk(out0, self.nb_grads, dim=1).indices).sum(dim=1)
            allowed = ((bits + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)  # the same 32 bits
        xa = x0.clone()
        iters = torch.zeros(b, dtype=torch.int32, device=x0.device)
        target = torch.full((b,), -1, dtype=torch.int32, device=x0.device)
        first = torch.full((b,), math.nan, device=x0.device)
        for it in range(self.max_iter):
            out = out0 if it == 0 else est.predict_device(xa, logits=self.on_logits, lengths=lt)
            jac = est.jacobian_device(xa, on_logits=self.on_logits, lengths=lt)
            dist, tgt, state = deepfool_step(jac, out, label, xa, self.norm, self.overshoot, clip, allowed)
            stepped = state == 1
            iters += stepped
            target = torch.where(stepped, tgt, target)
            if it == 0:
                first = dist
            if (it + 1) % self.CHECK_EVERY == 0 and it + 1 < self.max_iter and not bool(stepped.any()):
                break
        adv = xa if self.epsilon == 0 else torch.where(xa == x0, x0, x0 + (1.0 + self.epsilon) * (xa - x0))
        if clip is not None:
            adv = adv.clamp(*clip)
        if lt is not None:
            adv = torch.where(est.clip_mask(lt), adv, x0)
        final = est.predict_device(adv, logits=True, lengths=lt)
        return adv, iters, final.argmax(dim=1) != label, target, first

    def generate_device(self, xt, lengths=None):
        """x: float32 device tensor [B, n]; returns a NEW device tensor (the input is left untouched).  lengths (WaveformClassifier
        only): the samples of each row that belong to its clip."""
        from .extract_features_construct_dataset import JACOBIAN_CHUNK_BYTES

        est = self.estimator
        xt = est.rows_device(xt)
        b, n = xt.shape
        lt = est.lengths_device(lengths, b)
        chunk = min(max(1, JACOBIAN_CHUNK_BYTES // max(1, 4 * est.nb_classes * n)), int(est.batch_limit))
        parts = [self._chunk(xt[s:s + chunk], None if lt is None else lt[s:s + chunk]) for s in range(0, b, chunk)]
        if not parts:
            self.last = dict(iterations=np.zeros(0, dtype=np.int64), flipped=np.zeros(0, dtype=bool), target=np.zeros(0, dtype=np.int64),
                             first_dist=np.zeros(0))
            return xt.clone()
        cat = lambda i: torch.cat([p[i] for p in parts])
        self.last = dict(iterations=cat(1).cpu().numpy().astype(np.int64), flipped=cat(2).cpu().numpy(),
                         target=cat(3).cpu().numpy().astype(np.int64), first_dist=cat(4).double().cpu().numpy())
        return cat(0)

    def generate(self, x, lengths=None):
        """NumPy in, new NumPy out (the input is left untouched)."""
        adv = self.generate_device(_to_dev(x), lengths=lengths)
        return _as_given(adv, x)


def within_ball_device(adv, x, eps, norm, valid=None):
    """bool [B]: the perturbation of each row lies in the eps ball -- norm inf: per element eps plus one unit in the last place of
    the fp32 number |x| + eps; norm 2: eps (1 + 1e-6) + 1e-7; in fp64.  ``valid`` bool [B, n]: only those positions count."""
    d = adv.double() - x.double()
    if valid is not None:
        d = torch.where(valid, d, torch.zeros_like(d))
    e = float(np.float32(eps))
    if float(norm) == 2.0:
        return (d * d).sum(dim=1).sqrt() <= e * (1 + 1e-6) + 1e-7
    t = (x.double().abs() + float(eps)).float()
    room = e + (torch.nextafter(t, torch.full_like(t, math.inf)).double() - t.double())
    return (d.abs() <= room).all(dim=1)


class AutoAttack:
    """ART AutoAttack(estimator=, norm=, eps=, eps_step=, attacks=, batch_size=) (Croce & Hein 2020): an ensemble whose answer is
    the accuracy that survives every member.  ``attacks=None`` builds the list from this module's own classes at this ``eps``,
    ``norm`` and ``seed``: AutoProjectedGradientDescent with loss_type="cross_entropy", AutoProjectedGradientDescent with
    "difference_logits_ratio" (LEFT OUT below 3 classes, where that loss is undefined), DeepFool(norm=norm) and SquareAttack
    (LEFT OUT under norm=2: only its L-inf form is built).  ART's list is the same four with its own classes (restated from memory
    of its published implementation; ART is absent: parity unpinned).  ``norm``: np.inf or 2.  Ours, after the ``*``: ``seed`` (every
    member's), ``shape`` (SquareAttack's picture of a row; None: a strip) and ``targeted``: True is refused -- ART's form with one
    run per target class is not built.

    generate_device: labels are ``yt``, or the estimator's own predictions.  A row is ROBUST while the estimator's argmax equals
    its label; rows misclassified when clean are returned bit for bit.  Each attack in turn runs only on the rows that are still
    robust (gathering that subset, with its ``lengths``, is the one synchronisation per attack; a member's random draws are keyed
    by a row's position in the subset).  A row counts as broken only if the estimator's argmax at the result differs from the label
    AND the result lies in the ball (``within_ball_device``; only the clip's own samples count under ``lengths``) -- DeepFool's
    unbounded result passes or fails this check like any other.  A broken row keeps the first result that broke it; a row no attack
    broke is returned clean.  Afterwards: ``success_`` bool [B] (broken), ``broken_by_`` int32 [B] (the index into ``attacks``, -1
    never broken, -2 misclassified when clean) as device tensors and ``robust_accuracy_``, the share of all rows still robust."""

    def __init__(self, estimator, norm=np.inf, eps=0.3, eps_step=0.1, attacks=None, batch_size=32, *, seed=0, shape=None,
                 targeted=False):
        if not isinstance(estimator, (TensorFlowV2Classifier, WaveformClassifier)):
            raise TypeError("estimator must be a lipasr TensorFlowV2Classifier or WaveformClassifier")
        if targeted:
            raise ValueError("targeted=True: the targeted AutoAttack (one run per target class) is not built")
        self.norm = _norm_value(norm)
        if self.norm == 1.0:
            raise ValueError("norm=1: AutoAttack runs in norm 2 or np.inf")
        self.estimator, self.eps, self.eps_step = estimator, float(eps), float(eps_step)
        if not (0.0 <= self.eps < math.inf and 0.0 <= self.eps_step < math.inf):
            raise ValueError(f"eps = {eps}, eps_step = {eps_step}: finite, non-negative numbers are required")
        self.batch_size, self.seed, self.targeted = int(batch_size), int(seed), False
        if self.batch_size < 1:
            raise ValueError(f"batch_size = {batch_size}")
        if attacks is None:
            kw = dict(norm=norm, eps=self.eps, eps_step=self.eps_step, batch_size=self.batch_size, seed=self.seed)
            attacks = [AutoProjectedGradientDescent(estimator, loss_type="cross_entropy", **kw)]
            if estimator.nb_classes >= 3:
                attacks.append(AutoProjectedGradientDescent(estimator, loss_type="difference_logits_ratio", **kw))
            attacks.append(DeepFool(estimator, batch_size=self.batch_size, verbose=False, norm=norm))
            if self.norm == math.inf:
                attacks.append(SquareAttack(estimator, norm=np.inf, eps=self.eps, batch_size=self.batch_size, shape=shape, seed=self.seed))
        self.attacks = list(attacks)
        for a in self.attacks:
            if not callable(getattr(a, "generate_device", None)):
                raise TypeError(f"{type(a).__name__} has no generate_device")
        self.success_ = self.broken_by_ = self.robust_accuracy_ = None

    @staticmethod
    def _attack(attack, xs, ys, ls):
        import inspect

        takes = inspect.signature(attack.generate_device).parameters
        kw = {} if ls is None else dict(lengths=ls)
        return attack.generate_device(xs, ys, **kw) if "yt" in takes else attack.generate_device(xs, **kw)

    def generate_device(self, xt, yt=None, lengths=None):
        """xt: float32 device tensor [B, features or samples]; yt: one-hot [B, classes], class indices [B] or None; returns a NEW
        device tensor (the input is left untouched)."""
        est = self.estimator
        lt = est.lengths_device(lengths, len(xt))
        xt = est.rows_device(xt)
        b, dev = xt.shape[0], xt.device
        pred = est.predict_device(xt, logits=True, lengths=lt).argmax(dim=1) if b else torch.zeros(0, dtype=torch.int64, device=dev)
        if yt is None:
            labels = pred
        else:
            yt = yt.to(dev)
            labels = (yt.argmax(dim=1) if yt.dim() == 2 else yt).long()
            if tuple(labels.shape) != (b,):
                raise ValueError(f"y must be one-hot [B, classes] or class indices [B], got {tuple(yt.shape)}")
        robust = pred == labels
        adv = xt.clone()
        self.broken_by_ = torch.where(robust, -1, -2).to(torch.int32)
        mask_all = None if lt is None else est.clip_mask(lt)
        for i, attack in enumerate(self.attacks):
            idx = robust.nonzero()[:, 0]
            if idx.numel() == 0:
                break
            xs, ys = xt[idx].contiguous(), labels[idx]
            ls = None if lt is None else lt[idx].contiguous()
            cand = self._attack(attack, xs, ys, ls)
            moved = est.predict_device(cand, logits=True, lengths=ls).argmax(dim=1) != ys
            ok = moved & within_ball_device(cand, xs, self.eps, self.norm, None if mask_all is None else mask_all[idx])
            hit = idx[ok]
            adv[hit] = cand[ok]
            self.broken_by_[hit] = i
            robust[hit] = False
        self.success_ = self.broken_by_ >= 0
        self.robust_accuracy_ = float(robust.double().mean()) if b else 1.0
        return adv

    def generate(self, x, y=None, lengths=None):
        return generate_host(self, x, y, lengths)


class ImperceptibleASR:
    """ART ``ImperceptibleASR`` (Qin et al. 2019) over a WaveformClassifier, in either domain: a targeted attack in two stages.
    Stage 1 finds an adversarial perturbation inside an L-inf ball that shrinks while the attack succeeds (sign steps of
    ``learning_rate_1`` down CE(f(x0 + delta), y)); stage 2 pushes the perturbation's power spectrum under the clip's own
    masking threshold (plain gradient steps of ``learning_rate_2`` along g_net + alpha_u g_theta, L_theta and g_theta from
    ``PsychoacousticMasker.loss_gradient_device``), with alpha_u raised while the row stays adversarial and lowered while it is not.
    ``eps`` and the learning rates are amplitudes of this estimator's waveform and have no defaults (ART's are 16-bit sample
    units tuned for another model).  g_net is the gradient of each row's OWN cross-entropy (lipasr_mlp_input_grad's batch mean
    undone), so a row's path does not depend on the batch it runs in.

    A row's stage-1 result is x0 + delta at its last successful check (every ``num_iter_decrease_eps`` iterations), or x0 + its
    last delta if it never succeeded; |delta_u| <= ``last_eps[u]``, the ball that result was found in, and stage 2 stays inside it.
    Stage 2 keeps, per row, the adversarial iterate with the lowest L_theta seen at its checks (multiples of
    ``num_iter_increase_alpha`` / ``num_iter_decrease_alpha``), never one with a higher L_theta than the stage-1 result; it stops
    once every row has L_theta < ``loss_theta_min`` -- looked at only at multiples of ``num_iter_increase_alpha``, the one point
    where the loop returns to the host.  Afterwards: ``last_success`` (bool [B]), ``last_loss_theta_1`` / ``last_loss_theta``
    (L_theta after stage 1 / of the returned rows), ``last_eps``, ``last_stage1`` and ``last_iterate`` (device tensors)."""

    ALPHA_FLOOR = 0.0005

    def __init__(self, estimator, masker=None, *, eps, learning_rate_1, learning_rate_2, max_iter_1=1000, max_iter_2=4000,
                 loss_theta_min=0.05, decrease_factor_eps=0.8, num_iter_decrease_eps=10, alpha=0.05, increase_factor_alpha=1.2,
                 num_iter_increase_alpha=20, decrease_factor_alpha=0.8, num_iter_decrease_alpha=50, batch_size=32):
        from .psychoacoustic import PsychoacousticMasker

        if not isinstance(estimator, WaveformClassifier):
            raise TypeError("ImperceptibleASR runs over audio: the estimator must be a WaveformClassifier")
        if estimator.extractor.short_window:
            raise ValueError("ImperceptibleASR: the masker is built for the 2048 / 512 framing, not a short-window extractor")
        sr = 22050 if estimator.domain == "22k" else int(estimator.extractor.sr_in)
        self.estimator = estimator
        self.masker = masker if masker is not None else PsychoacousticMasker(sample_rate=sr, device=estimator.extractor.device)
        if not isinstance(self.masker, PsychoacousticMasker):
            raise TypeError("masker must be a lipasr.psychoacoustic.PsychoacousticMasker")
        for name, v in (("eps", eps), ("learning_rate_1", learning_rate_1), ("learning_rate_2", learning_rate_2)):
            if not (float(v) > 0):
                raise ValueError(f"{name}={v!r} must be positive")
        for name, v in (("max_iter_1", max_iter_1), ("max_iter_2", max_iter_2)):
            if int(v) < 0:
                raise ValueError(f"{name}={v!r} must not be negative")
        for name, v in (("num_iter_decrease_eps", num_iter_decrease_eps), ("num_iter_increase_alpha", num_iter_increase_alpha),
                        ("num_iter_decrease_alpha", num_iter_decrease_alpha), ("batch_size", batch_size)):
            if int(v) < 1:
                raise ValueError(f"{name}={v!r} must be at least 1")
        self.eps, self.learning_rate_1, self.learning_rate_2 = float(eps), float(learning_rate_1), float(learning_rate_2)
        self.max_iter_1, self.max_iter_2, self.loss_theta_min = int(max_iter_1), int(max_iter_2), float(loss_theta_min)
        self.decrease_factor_eps, self.num_iter_decrease_eps = float(decrease_factor_eps), int(num_iter_decrease_eps)
        self.alpha, self.increase_factor_alpha, self.num_iter_increase_alpha = float(alpha), float(increase_factor_alpha), int(num_iter_increase_alpha)
        self.decrease_factor_alpha, self.num_iter_decrease_alpha = float(decrease_factor_alpha), int(num_iter_decrease_alpha)
        self.batch_size = int(batch_size)
        self.targeted = True
        self.last_success = self.last_loss_theta = self.last_loss_theta_1 = self.last_eps = self.last_stage1 = self.last_iterate = None

    def _hit(self, xa, target):
        return self.estimator.predict_device(xa, logits=True).argmax(dim=1) == target

    def _stage1(self, x0, yb, target):
        """-> (result, success, eps of the ball the result lies in)."""
        est, mk = self.estimator, self.masker
        b = x0.shape[0]
        delta, xa, g = torch.zeros_like(x0), x0.clone(), torch.empty_like(x0)
        eps_u = torch.full((b,), self.eps, device=x0.device)
        res, eps_res = x0.clone(), eps_u.clone()
        succ = torch.zeros(b, dtype=torch.bool, device=x0.device)
        for it in range(1, self.max_iter_1 + 1):
            est.loss_gradient_device(xa, yb, out=g)
            mk.step_device(delta, xa, x0, g, None, None, eps_u, self.learning_rate_1, True, est.clip_values)
            if it % self.num_iter_decrease_eps == 0:
                ok = self._hit(xa, target)
                res = torch.where(ok[:, None], xa, res)
                eps_res = torch.where(ok, eps_u, eps_res)
                succ |= ok
                eps_u = torch.where(ok, self.decrease_factor_eps * torch.minimum(eps_u, delta.abs().amax(dim=1)), eps_u)
        never = ~succ
        res = torch.where(never[:, None], xa, res)
        eps_res = torch.where(never, eps_u, eps_res)
        return res, succ, eps_res

    def _stage2(self, x0, yb, target, x1, succ, eps_u):
        """-> (result, success, L_theta after stage 1, L_theta of the result, the last iterate)."""
        est, mk = self.estimator, self.masker
        b = x0.shape[0]
        theta, psd_max = mk.prepare_device(x0)
        xa = x1.clone()
        delta = xa - x0
        g, gt = torch.empty_like(x0), torch.empty_like(x0)
        loss1, _ = mk.loss_gradient_device(delta, theta, psd_max, need_grad=False)
        best, best_loss, succ = x1.clone(), loss1.clone(), succ.clone()
        alpha = torch.full((b,), self.alpha, device=x0.device)
        # lipasr_mlp_input_grad differentiates the batch MEAN: lr (b g + alpha g_theta) = (lr b) (g + (alpha / b) g_theta)
        alpha_b, lr = alpha / b, self.learning_rate_2 * b
        inc, dec = self.num_iter_increase_alpha, self.num_iter_decrease_alpha
        for it in range(1, self.max_iter_2 + 1):
            est.loss_gradient_device(xa, yb, out=g)
            mk.loss_gradient_device(delta, theta, psd_max, out=gt)
            mk.step_device(delta, xa, x0, g, gt, alpha_b, eps_u, lr, False, est.clip_values)
            if it % inc and it % dec:
                continue
            ok = self._hit(xa, target)
            cur, _ = mk.loss_gradient_device(delta, theta, psd_max, need_grad=False)
            better = ok & (cur < best_loss)
            best = torch.where(better[:, None], xa, best)
            best_loss = torch.where(better, cur, best_loss)
            succ |= better
            if it % inc == 0:
                alpha = torch.where(ok, alpha * self.increase_factor_alpha, alpha)
            if it % dec == 0:
                alpha = torch.where(ok, alpha, (alpha * self.decrease_factor_alpha).clamp_min(self.ALPHA_FLOOR))
            alpha_b = alpha / b
            if it % inc == 0 and bool((best_loss < self.loss_theta_min).all()):
                break
        return best, succ, loss1, best_loss, xa

    def generate_device(self, xt, yt=None, lengths=None):
        """xt: float32 device tensor [B, n] of clips of ONE length, yt: one-hot targets [B, classes]; returns a NEW tensor."""
        if lengths is not None:
            raise ValueError("lengths=: ImperceptibleASR takes clips of one length (the masker has no per-clip lengths)")
        if yt is None:
            raise ValueError("Target labels `y` need to be provided for a targeted attack.")
        est = self.estimator
        xt = est.rows_device(xt)
        if tuple(yt.shape) != (xt.shape[0], est.nb_classes):
            raise ValueError(f"y must be one-hot [{xt.shape[0]}, {est.nb_classes}]")
        bs = min(self.batch_size, est.batch_limit)
        out, keep = torch.empty_like(xt), {k: [] for k in ("succ", "l1", "l2", "eps", "x1", "it")}
        for s in range(0, xt.shape[0], bs):
            x0 = xt[s:s + bs].contiguous()
            yb = yt[s:s + bs].to(torch.float32).contiguous()
            target = yb.argmax(dim=1)
            x1, succ, eps_u = self._stage1(x0, yb, target)
            best, succ, l1, l2, last = self._stage2(x0, yb, target, x1, succ, eps_u)
            out[s:s + bs] = best
            for k, v in zip(("succ", "l1", "l2", "eps", "x1", "it"), (succ, l1, l2, eps_u, x1, last)):
                keep[k].append(v)
        cat = lambda k: torch.cat(keep[k])
        self.last_success, self.last_loss_theta_1, self.last_loss_theta = cat("succ").cpu().numpy(), cat("l1").cpu().numpy(), cat("l2").cpu().numpy()
        self.last_eps, self.last_stage1, self.last_iterate = cat("eps").cpu().numpy(), cat("x1"), cat("it")
        return out

    def generate(self, x, y=None, lengths=None):
        if lengths is not None:
            raise ValueError("lengths=: ImperceptibleASR takes clips of one length (the masker has no per-clip lengths)")
        if y is None:
            raise ValueError("Target labels `y` need to be provided for a targeted attack.")
        adv = self.generate_device(_to_dev(x), _to_dev(y))
        return _as_given(adv, x)


def sign_step(x_adv, x0, g, alpha, eps):
    """Stand-alone K4 on device tensors, in place on x_adv."""
    h = N.get_handle(x_adv.device.index)
    N.check(N.lib.lipasr_sign_step(h.h, N.ptr(x_adv), N.ptr(x0), N.ptr(g), x_adv.numel(), float(alpha), float(eps), N.stream_ptr()))
    return x_adv


def lp_step(x_adv, x0, g, alpha, eps, norm):
    """Stand-alone K4 in any norm (lipasr_lp_step) on device tensors [rows, n] (or [n]), in place on x_adv: ART's step
    x' = x_adv + alpha d(g) and projection onto the eps ball around x0; alpha < 0 is the targeted step, eps = inf no projection."""
    h = N.get_handle(x_adv.device.index)
    rows, n = (1, x_adv.numel()) if x_adv.dim() == 1 else (x_adv.shape[0], x_adv[0].numel())
    N.check(N.lib.lipasr_lp_step(h.h, N.ptr(x_adv), N.ptr(x0), N.ptr(g), rows, n, _norm_value(norm), float(alpha), float(eps),
                                 N.stream_ptr()))
    return x_adv


# ------------------------------------------------------------------------------------------------ A12 (device noise)
_noise_calls = [0]


def _noise(arr, mode, p0, p1, seed):
    was_tensor = torch.is_tensor(arr)
    t = _to_dev(arr).clone()
    one_d = t.dim() == 1
    if one_d:
        t = t[None, :]
    if seed is None:
        _noise_calls[0] += 1
        seed = 0xA77AC000 + _noise_calls[0]
    h = N.get_handle(t.device.index)
    N.check(N.lib.lipasr_add_noise_f32(h.h, N.ptr(t), t.shape[0], t.shape[1], mode, float(p0), float(p1), int(seed), N.stream_ptr()))
    if one_d:
        t = t[0]
    return t if was_tensor else t.cpu().numpy()


def add_white_noise(array, sigma, seed=None):
    """attacks.py:73-86: array + N(0, sigma)."""
    return _noise(array, 0, sigma, 0.0, seed)


def add_noise(x, p, alpha, seed=None):
    """attacks.py:166-183 (mixtgauss :145-163): impulse mixture, sigma0 = alpha, sigma1 = 10 alpha, peaks where |N(0,1)| < p."""
    return _noise(x, 1, p, alpha, seed)


def add_white_noise_with_snr(audio, target_snr_db, seed=None):
    """attacks.py:222-245: white noise whose power sits target_snr_db below the clip's mean power."""
    return _noise(audio, 2, target_snr_db, 0.0, seed)


def add_white_noise_on_dataset(dataset, sigma, seed=None):
    """attacks.py:186-201: white noise on every row of an MFCC matrix."""
    return _noise(dataset, 0, sigma, 0.0, seed)


def add_noise_mixture_on_dataset(dataset, p, alpha, seed=None):
    """attacks.py:204-219."""
    return _noise(dataset, 1, p, alpha, seed)


def noisy_audio_to_mfcc(waves, sr_in=16000, sigma=0, p=0, alpha=0, target_snr_db=None, seed=None, utterance_length=44):
    """The one end-to-end audio flow of the reference (attacks.py:89-121, 248-274) for a batch of clips:
    resample -> add noise at 22 050 Hz -> MFCC -> (B, 20*utterance_length) device tensor."""
    w = _to_dev(waves)
    ex = _extractor(int(sr_in), w.shape[1], w.shape[0])
    y = ex.resample(w)
    if target_snr_db is not None:
        y = add_white_noise_with_snr(y, target_snr_db, seed)
    elif sigma != 0:
        y = add_white_noise(y, sigma, seed)
    elif p != 0 and alpha != 0:
        y = add_noise(y, p, alpha, seed)
    return ex.from_22k(y, utterance_length)


def _files_to_batches(filenames):
    groups = {}
    for i, fn in enumerate(filenames):
        x, sr = read_wav(fn)
        groups.setdefault((sr, len(x)), []).append((i, x))
    return groups


def black_box_attack_on_audio_dataset(filenames, sigma, p, alpha, seed=None):
    """attacks.py:124-142: noisy MFCC for a list of wav files, (N, 880) float64."""
    out = np.zeros((len(filenames), 20 * 44))
    for (sr, n), items in _files_to_batches(filenames).items():
        w = np.stack([x for _, x in items])
        f = noisy_audio_to_mfcc(w, sr, sigma=sigma, p=p, alpha=alpha, seed=seed).cpu().numpy()
        for (i, _), row in zip(items, f):
            out[i] = row
    return out


def black_box_attack_on_audio_dataset_snr(filenames, target_snr_db, seed=None):
    """attacks.py:277-294."""
    out = np.zeros((len(filenames), 20 * 44))
    for (sr, n), items in _files_to_batches(filenames).items():
        w = np.stack([x for _, x in items])
        f = noisy_audio_to_mfcc(w, sr, target_snr_db=target_snr_db, seed=seed).cpu().numpy()
        for (i, _), row in zip(items, f):
            out[i] = row
    return out


def black_box_attack_on_audio(file_path, utterance_length, sigma=0, p=0, alpha=0, seed=None):
    """attacks.py:89-121: one file -> noisy MFCC (20, utterance_length), float32 NumPy."""
    x, sr = read_wav(file_path)
    f = noisy_audio_to_mfcc(x[None, :], sr, sigma=sigma, p=p, alpha=alpha, seed=seed, utterance_length=utterance_length)
    return f.view(20, utterance_length).cpu().numpy()


def black_box_attack_on_audio_snr(file_path, utterance_length, target_snr_db, seed=None):
    """attacks.py:248-274."""
    x, sr = read_wav(file_path)
    f = noisy_audio_to_mfcc(x[None, :], sr, target_snr_db=target_snr_db, seed=seed, utterance_length=utterance_length)
    return f.view(20, utterance_length).cpu().numpy()


def mixtgauss(N_, p, sigma0, sigma1, seed=None):
    """attacks.py:145-163: N_ samples of the impulse mixture (sigma1 where |N(0,1)| < p, sigma0 elsewhere), drawn by the
    device generator -- add_noise's noise term on its own."""
    if abs(sigma1 - 10 * sigma0) > 1e-12 * max(1.0, abs(sigma1)):
        raise NotImplementedError("mixtgauss with sigma1 != 10 sigma0 (the reference's only call, attacks.py:178-180, uses 10x)")
    z = torch.zeros(int(N_), device=_dev())
    h = N.get_handle(z.device.index)
    if seed is None:
        _noise_calls[0] += 1
        seed = 0xA77AC000 + _noise_calls[0]
    N.check(N.lib.lipasr_add_noise_f32(h.h, N.ptr(z), 1, z.numel(), 1, float(p), float(sigma0), int(seed), N.stream_ptr()))
    return z.cpu().numpy()


def load_npy_dataset(path):
    """attacks.py:27-45: the six ``.npy`` files of a processed dataset folder (``path`` ends with a separator, as in the
    reference's call sites)."""
    import os

    def ld(name):
        return np.load(os.path.join(path, name) if os.path.isdir(path) else path + name)

    return (ld("train_data.npy"), ld("train_label.npy"), ld("dev_data.npy"), ld("dev_label.npy"), ld("test_data.npy"),
            ld("test_label.npy"))
