"""The genetic black-box attack of Alzantot, Balaji and Srivastava (2018, "Did you hear that? Adversarial examples against
automatic speech recognition") over the estimators of lipasr.estimators: it queries scores only, never a gradient.

Why it is here: a query-only attack that beats the gradient attacks at the same eps says that the gradients are masked (Athalye et
al. 2018; Carlini et al. 2019) -- and a constrained network (NonNeg kernels, a small Lipschitz constant, a saturating softmax) is
where that can happen.  It is also an empirical upper bound on the radii of get_robustness_radius and Smooth.certify that does
not rest on those gradients.

Per clip a population of ``pop_size`` perturbed copies inside the L-inf ball of radius eps.  One generation, per chunk of at most
``estimator.batch_limit // pop_size`` clips: the estimator's ``predict_device(..., logits=True)`` scores every member,
lipasr_genetic_select turns the scores into fitness, elite and parent pairs (drawn with probability softmax(fitness / T)), and
lipasr_genetic_breed writes the children into the other of two buffers (crossover element by element, a mutation of a small share
of the elements, the clamp to the ball and to the clip range).  Two launches of ours per generation; the only synchronisation is
``done.all()`` every ``check_every`` generations.  Philox counters are keyed by seed, clip, generation, member and element, so a
clip's run depends on neither its neighbours nor the chunking.  include/lipasr.h fixes the conventions.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from ._rows import _dev_tensor, check_estimator, clip_pair, generate_host, labels_device, resolve_clip_values, rows2d


def mutate_threshold(mutation_p):
    """round(p * 2^24): the integer lipasr_genetic_breed compares 24 random bits with."""
    p = float(mutation_p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"mutation_p = {mutation_p}: a probability is required")
    return int(round(p * 16777216.0))


def genetic_breed(x0, pop, generation, seed, mutate_thresh, step, eps, *, pop_in=None, parents=None, n_valid=None, clip0=0,
                  clip_values=None, out=None):
    """lipasr_genetic_breed on device tensors: x0 float32 [B, n]; pop_in float32 [B * pop, n] with parents int32 [B, pop, 2], or
    neither (the initial population); n_valid int32 [B] or None -> float32 [B * pop, n], row b * pop + p child p of clip
    ``clip0 + b``."""
    b, n = rows2d(x0, "x0")
    pop, generation = int(pop), int(generation)
    if not 0 <= generation < 1 << 24:
        raise ValueError(f"generation = {generation}: 0 to 2^24 - 1")
    if not 0 <= int(mutate_thresh) <= 1 << 24:
        raise ValueError(f"mutate_thresh = {mutate_thresh}: 0 to 2^24")
    if pop_in is not None:
        _dev_tensor(pop_in, torch.float32, (b * pop, n), "pop_in")
    if parents is not None:
        _dev_tensor(parents, torch.int32, (b, pop, 2), "parents")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")
    if out is None:
        out = torch.empty(b * max(pop, 0), n, device=x0.device)
    else:
        _dev_tensor(out, torch.float32, (b * pop, n), "out")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x0.device.index)
    N.check(N.lib.lipasr_genetic_breed(h.h, N.ptr(x0), N.ptr(n_valid), N.ptr(pop_in), N.ptr(parents), b, pop, n, int(clip0), generation,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(mutate_thresh), float(step), float(eps), lo, hi, N.ptr(out),
                                       N.stream_ptr()))
    return out


def genetic_select(logits, labels, pop, generation, seed, temperature, *, targeted=False, clip0=0, fitness, best, done, parents):
    """lipasr_genetic_select on device tensors: logits float32 [B * pop, C], labels int32 [B]; writes fitness float32 [B, pop], best
    int32 [B], done int32 [B] (sticky; generation + 1 where the clip succeeds) and parents int32 [B, pop, 2]."""
    rows, c = rows2d(logits, "logits", "[B * pop, classes]")
    pop, generation = int(pop), int(generation)
    if pop < 1 or rows % pop:
        raise ValueError(f"{rows} rows of logits are no multiple of pop = {pop}")
    if not 0 <= generation < 1 << 24:
        raise ValueError(f"generation = {generation}: 0 to 2^24 - 1")
    b = rows // pop
    _dev_tensor(labels, torch.int32, (b,), "labels")
    _dev_tensor(fitness, torch.float32, (b, pop), "fitness")
    _dev_tensor(best, torch.int32, (b,), "best")
    _dev_tensor(done, torch.int32, (b,), "done")
    _dev_tensor(parents, torch.int32, (b, pop, 2), "parents")
    h = N.get_handle(logits.device.index)
    N.check(N.lib.lipasr_genetic_select(h.h, N.ptr(logits), N.ptr(labels), b, pop, c, 1 if targeted else 0, float(temperature), int(clip0),
                                        generation, int(seed) & 0xFFFFFFFFFFFFFFFF, N.ptr(fitness), N.ptr(best), N.ptr(done),
                                        N.ptr(parents), N.stream_ptr()))


class GeneticAttack:
    """The genetic algorithm of Alzantot et al. (2018) in the L-inf ball of radius ``eps`` around every row: over the features of a
    TensorFlowV2Classifier, or over the samples of a WaveformClassifier (either domain; ``lengths=`` as there: the perturbation
    stays inside each clip and the rest of the row is returned bit for bit; a short-window extractor takes no lengths).

    ``pop_size`` (2 .. 64), ``mutation_p`` (the share of elements that mutate in a child) and ``temperature`` (of the softmax
    over the fitness that draws the parents) default to the paper's settings AS REMEMBERED -- population 20, mutation
    probability 0.0005, temperature 0.01; nothing in this repository can check them against the paper, so they are keywords.
    ``step``: the largest mutation, uniform in (-step, step]; None: eps.  ``max_iter``: the generations evaluated at most, so at
    most pop_size * max_iter queries per clip.  ``targeted``: y holds the class to reach (required then); otherwise the class to
    leave, y=None: the model's own prediction.  Fitness is the logit margin: max_{c != y} z_c - z_y (targeted: its negative);
    a clip is done when a member's is positive, and its population is frozen from then on.
    ``seed``: the Philox key; a clip's draws are a function of (seed, its row index in x, generation, member, element).
    ``clip_values``: (lo, hi) clamps every member; default: the estimator's (a TensorFlowV2Classifier has none).
    ``check_every``: the generations between two looks at ``done`` -- the only synchronisation.

    After generate / generate_device: ``success_`` bool [B], ``queries_`` int64 [B] (pop_size x the generations evaluated until the
    clip was done, or all of them), ``fitness_`` float32 [B] (of the returned member), as device tensors."""

    _UNSET = object()

    def __init__(self, estimator, eps, *, pop_size=20, max_iter=500, mutation_p=0.0005, step=None, temperature=0.01, targeted=False,
                 seed=0, clip_values=_UNSET, check_every=10):
        check_estimator(estimator)
        self.estimator = estimator
        self.eps = float(eps)
        self.step = self.eps if step is None else float(step)
        if not (0.0 <= self.eps < math.inf and 0.0 <= self.step < math.inf):
            raise ValueError(f"eps = {eps}, step = {step}: finite, non-negative numbers are required")
        self.pop_size, self.max_iter, self.check_every = int(pop_size), int(max_iter), int(check_every)
        if not 2 <= self.pop_size <= 64:
            raise ValueError(f"pop_size = {pop_size}: 2 to 64 are supported")
        if not 1 <= self.max_iter <= 1 << 24:
            raise ValueError(f"max_iter = {max_iter}: 1 to 2^24")
        if self.check_every < 1:
            raise ValueError(f"check_every = {check_every}")
        self.mutation_p, self._thresh = float(mutation_p), mutate_threshold(mutation_p)
        self.temperature = float(temperature)
        if not 0.0 < self.temperature < math.inf:
            raise ValueError(f"temperature = {temperature}: a finite, positive number is required")
        self.targeted, self.seed = bool(targeted), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.clip_values = resolve_clip_values(estimator, clip_values, GeneticAttack._UNSET)
        self.success_ = self.queries_ = self.fitness_ = None

    def generate_device(self, xt, yt=None, lengths=None):
        """xt: float32 device tensor [B, features or samples]; yt: one-hot [B, classes] or class indices [B] or None; returns a NEW
        device tensor: per clip member ``best`` of the last population evaluated -- the adversarial one where the clip is done,
        the fittest otherwise."""
        est, P = self.estimator, self.pop_size
        xt = est.rows_device(xt)
        b, n = xt.shape
        dev = xt.device
        lt = est.lengths_device(lengths, b)
        pos = None if lt is None else est.clip_mask(lt).sum(dim=1).to(torch.int32).contiguous()
        labels = labels_device(xt, yt, self.targeted, lambda: est.predict_device(xt, logits=True, lengths=lt).argmax(dim=1))
        adv = xt.clone()
        self.success_ = torch.zeros(b, dtype=torch.bool, device=dev)
        self.queries_ = torch.zeros(b, dtype=torch.int64, device=dev)
        self.fitness_ = torch.full((b,), -math.inf, device=dev)
        if b == 0 or n == 0:
            return adv
        bc = max(1, int(est.batch_limit) // P)
        bufs = [torch.empty(min(b, bc) * P, n, device=dev) for _ in range(2)]
        for s in range(0, b, bc):
            x0 = xt[s:s + bc]
            bb = x0.shape[0]
            nv = None if pos is None else pos[s:s + bb]
            lrep = None if lt is None else lt[s:s + bb].repeat_interleave(P)
            lab = labels[s:s + bb]
            fitness = torch.empty(bb, P, device=dev)
            best = torch.zeros(bb, dtype=torch.int32, device=dev)
            done = torch.zeros(bb, dtype=torch.int32, device=dev)
            parents = torch.empty(bb, P, 2, dtype=torch.int32, device=dev)
            kw = dict(n_valid=nv, clip0=s, clip_values=self.clip_values)
            cur = genetic_breed(x0, P, 0, self.seed, self._thresh, self.step, self.eps, out=bufs[0][:bb * P], **kw)
            nxt = bufs[1][:bb * P]
            evaluated = 0
            for g in range(self.max_iter):
                genetic_select(est.predict_device(cur, logits=True, lengths=lrep), lab, P, g, self.seed, self.temperature,
                               targeted=self.targeted, clip0=s, fitness=fitness, best=best, done=done, parents=parents)
                evaluated = g + 1
                if evaluated == self.max_iter or (evaluated % self.check_every == 0 and bool((done != 0).all())):
                    break
                genetic_breed(x0, P, g + 1, self.seed, self._thresh, self.step, self.eps, pop_in=cur, parents=parents, out=nxt, **kw)
                cur, nxt = nxt, cur
            idx = best.long()
            rows = torch.arange(bb, device=dev)
            adv[s:s + bb] = cur.view(bb, P, n)[rows, idx]
            self.success_[s:s + bb] = done != 0
            self.queries_[s:s + bb] = P * torch.where(done != 0, done, torch.full_like(done, evaluated)).long()
            self.fitness_[s:s + bb] = fitness[rows, idx]
        return adv

    def generate(self, x, y=None, lengths=None):
        return generate_host(self, x, y, lengths)
