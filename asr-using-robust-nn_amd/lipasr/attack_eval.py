"""The evaluation script at the bottom of attacks.py (:296-693) without its ``input()`` prompts: each prompt is an
argument, each branch one accuracy-vs-strength sweep over a constrained and an unconstrained model.  The sweeps only
orchestrate -- noise, MFCC, gradients and attacks are the kernels behind ``lipasr.attacks``.  Plotting (matplotlib
windows) is left to the caller: every sweep returns ``(grid, {model name: accuracies})``.

    prompt in attacks.py                                   argument here
    "standardized before or after the attack? [B]/[A]"     standardize="before" | "after"          (:320-322)
    "Black-box or white-box attack? [B]/[W]"               attack="black" | "white"                (:324)
    "[S]imple/[M]ixture/[SNR]"                             kind="simple" | "mixture" | "snr"       (:326)
    "noise over [A]udio or [M]FCC"                         over="audio" | "mfcc"                   (:327)
    "[F]GSM/Carlini[L2]/Carlini[Linf]/[P]GD/[J]SMA"        kind="fgsm" | "l2" | "linf" | "pgd" | "jsma"   (:494)
    (no prompt: ART's norm keyword of FGM / PGD)           --norm inf | 1 | 2 (default inf, the reference's)
    (no prompt: dolphin_attack.m + a microphone model)     attack="dolphin": accuracy against the carrier level
    (no prompt: the Lipschitz read-outs, global and local) attack="lipschitz": lipschitz_report over="mfcc" | "audio"
    (no prompt: certified radius next to DeepFool's)       attack="radius": radius_report over="mfcc" | "audio", --norm 2 | inf
    (no prompt: certified accuracy by bound propagation)   attack="certify": certify_report --norm inf | 2, --method ibp | crown-ibp
    (no prompt: Auto-PGD, per-row step control, CE or DLR) attack="white", kind="apgd", --loss ce | dlr, --norm inf | 2, over="mfcc" | "audio"
    (no prompt: the genetic query-only attack)             attack="black", kind="genetic": genetic_sweep over="mfcc" | "audio"
    (no prompt: Square Attack, one score query per step)   attack="black", kind="square": square_sweep over="mfcc" | "audio"
    (no prompt: HopSkipJump, the label only, min. norm)    attack="black", kind="hsj", --norm inf | 2: hopskipjump_sweep over="mfcc" | "audio"
    (no prompt: the AutoAttack ensemble, robust accuracy)  attack="white", kind="auto", --norm inf | 2, over="mfcc" | "audio"
    (no prompt: randomized smoothing, CERTIFY per clip)    attack="smooth":smooth_report over="mfcc" | "audio", --sigma S [--n0 --n --alpha]
    (no prompt: the attack played in a room, EOT)          attack="white" | "black", over="audio", --room R [--room-taps --room-t60 LO HI --room-seed]:
                                                           over_the_air_sweep, kind="fgsm" | "pgd" | "apgd" | "auto" | "genetic" | "square"
    (no prompt: one noise vector for every clip)           attack="white", kind="universal", --norm inf | 2, over="mfcc" | "audio" [--shift --length P
                                                           --max-iter E --room R]: universal_sweep, fitted on one half, heard on the other
    (no prompt: worst-case delay, speed and level)         attack="black" (the grid alone) | "white" (--refine N), kind="warp", over="audio"
                                                           [--max-shift-ms D ... --max-rate R --max-gain-db G --room R]: time_warp_sweep
    (no prompt: a defence that cleans the input)           attack="white" | "black", over="audio", --defence median:5,lowpass:4000:101,quantize:8
                                                           [--defence-backward chain | identity --detect-fpr F]: defended_sweep, the kinds of --room
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from . import attacks as A
from .extract_features_construct_dataset import (get_lipschitz_bound, get_lipschitz_constrained, get_local_lipschitz, get_norms,
                                                  get_robustness_radius, get_upper_lipschitz)
from .keras import CategoricalCrossentropy, load_model, to_categorical

# the grids the reference hard-codes
AUDIO_SIGMAS = [0, 0.002, 0.004, 0.01, 0.015, 0.02, 0.03, 0.04, 0.05, 0.075, 0.1]  # :329
AUDIO_ALPHAS = np.linspace(0, 0.015, 15)                                              # :313
SNRS = [60, 30, 20, 15, 10, 5, 0]                                                     # :311
MFCC_SIGMAS = np.linspace(0, 100, 20)                                                 # :312
MFCC_ALPHAS = np.linspace(0, 100, 30)                                                 # :452
MIXTURE_P = 0.01                                                                      # :355, :451
# ours (the reference has no such sweep): the constant added to the normalised voice before the carrier multiplies it --
# dolphin_attack.m's 0.001 first, the DolphinAttack paper's 1 last
DOLPHIN_CARRIER_LEVELS = [0.001, 0.01, 0.1, 0.3, 1.0]
# ours: the largest delay either way of time_warp_sweep, in milliseconds (100 ms is the shift augmentation of Speech Commands)
WARP_SHIFTS_MS = [0, 2, 5, 10, 20, 50, 100]


def accuracy(predictions, labels_onehot):
    """np.sum(argmax(pred) == argmax(labels)) / len(labels) (:337-338)."""
    return float(np.sum(np.argmax(predictions, axis=1) == np.argmax(labels_onehot, axis=1)) / len(labels_onehot))


def _tag(name):
    """What a printed line says after its subject: nothing for the constrained model, the name of any other."""
    return "" if name == "constrained" else " " + name


def _sweep(models, grid, make_data, labels, what):
    acc = {name: [] for name in models}
    for item in grid:
        for name, model in models.items():
            a = accuracy(model.predict(make_data(name, model, item)), labels)
            acc[name].append(a)
            print(f"Accuracy on {what} test examples{_tag(name)}: {a * 100}% ({item})")
    return list(grid), {k: np.asarray(v) for k, v in acc.items()}


def black_box_sweep(models, train_data, val_data, test_data, test_labels, kind="simple", over="mfcc", standardize="before",
                    test_filenames=None, grid=None, points=None, seed=None):
    """attacks.py:326-491.  ``models``: {"constrained": model, "unconstrained": model}; data as load_npy_dataset returns
    it; ``test_labels`` one-hot.  Noise over audio re-extracts the MFCCs of ``test_filenames`` and standardizes them with
    the statistics of (train, val, noisy test) exactly as :333 does."""
    if standardize == "before" and over == "mfcc":
        train_data, val_data, test_data = A.standardize_dataset(train_data, val_data, test_data)
    if over == "audio":
        if test_filenames is None:
            raise ValueError("noise over audio needs test_filenames (test_dataset_to_add_noise/test_filenames.npy)")
        if standardize == "before":
            train_data, val_data, _ = A.standardize_dataset(train_data, val_data, test_data)  # :320-322 precede the sweep
        grid = grid if grid is not None else {"simple": AUDIO_SIGMAS, "mixture": AUDIO_ALPHAS, "snr": SNRS}[kind]

        def make(name, model, item):
            if kind == "simple":
                d = A.black_box_attack_on_audio_dataset(test_filenames, item, p=0, alpha=0, seed=seed)
            elif kind == "mixture":
                d = A.black_box_attack_on_audio_dataset(test_filenames, sigma=0, p=MIXTURE_P, alpha=item, seed=seed)
            else:
                d = A.black_box_attack_on_audio_dataset_snr(test_filenames, item, seed=seed)
            return A.standardize_dataset(train_data, val_data, d)[2]
    elif over == "mfcc":
        if kind == "snr":
            raise ValueError("the SNR attack is defined on audio only (attacks.py:391)")
        grid = grid if grid is not None else {"simple": MFCC_SIGMAS, "mixture": MFCC_ALPHAS}[kind]

        def make(name, model, item):
            d = (A.add_white_noise_on_dataset(test_data, item, seed=seed) if kind == "simple"
                 else A.add_noise_mixture_on_dataset(dataset=test_data, p=MIXTURE_P, alpha=item, seed=seed))
            return A.standardize_dataset(train_data, val_data, d)[2] if standardize == "after" else d
    else:
        raise ValueError("over must be 'audio' or 'mfcc'")
    return _sweep(models, list(grid)[:points], make, test_labels, "black-box attack")


def _padded_rows(items, n_pad, lens):
    """[(file index, samples)] -> (float32 device tensor [len(items), n_pad], zero-padded rows; int32 device lengths)."""
    w = np.zeros((len(items), n_pad), dtype=np.float32)
    for r, (_, x) in enumerate(items):
        w[r, :len(x)] = x
    return A._to_dev(w), torch.as_tensor(lens).to(A._dev())


def _audio_work(models, train_data, val_data, test_filenames):
    """What the sweeps and read-outs over the audio of ``test_filenames`` share -> (work, scaler, bmax): the files grouped into
    batches [(rate, row length, [(file index, samples)], per-clip lengths or None)], and the StandardScaler fitted on (train, val,
    the files' clean MFCCs); train and val as _TestRows hands them on."""
    groups = A._files_to_batches(test_filenames)
    # A rate whose files differ in length goes through ONE extractor and one WaveformClassifier per model, the clips side by
    # side with lengths= (16 kHz and 8 kHz: the rates whose plans take per-clip lengths); rows are padded to the longest clip
    # rounded up to a multiple of 4000 samples, compute_mfcc_all_files' rule, so that the plans are the ones extraction made.
    # A rate with one length, and every other rate, keeps one group per (rate, length).
    n_lengths = {}
    for (sr, n) in groups:
        n_lengths[sr] = n_lengths.get(sr, 0) + 1
    ragged = {}  # sr -> [(file index, samples)] in file order
    for (sr, n), items in groups.items():
        if sr in (16000, 8000) and n_lengths[sr] > 1:
            ragged.setdefault(sr, []).extend(items)
    work = [(sr, n, items, None) for (sr, n), items in groups.items() if sr not in ragged]
    bmax = min(m._max_batch for m in models.values()) if models else 1
    for sr, items in ragged.items():
        items.sort(key=lambda it: it[0])
        lens = np.array([len(x) for _, x in items], dtype=np.int32)
        n_pad = -(-int(lens.max()) // 4000) * 4000
        work.append((sr, n_pad, items, lens))
    # the statistics black_box_sweep(over="audio") uses at sigma = 0: those of (train, val, the files' clean MFCCs)
    if not ragged:
        clean = A.black_box_attack_on_audio_dataset(test_filenames, 0, p=0, alpha=0)
    else:
        clean = np.zeros((len(test_filenames), 20 * 44))
        for sr, n, items, lens in work:
            idx = [i for i, _ in items]
            if lens is None:
                clean[idx] = A.noisy_audio_to_mfcc(np.stack([x for _, x in items]), sr).cpu().numpy()
                continue
            w, lt = _padded_rows(items, n, lens)
            ex = A._extractor(int(sr), int(n), min(w.shape[0], bmax))
            clean[idx] = torch.cat([ex(w[s:s + ex.batch_max], 44, n_valid=lt[s:s + ex.batch_max])
                                    for s in range(0, w.shape[0], ex.batch_max)]).cpu().numpy()
    sc = A.StandardScaler().fit(np.concatenate([np.asarray(train_data), np.asarray(val_data), clean]))
    return work, sc, bmax


def _audio_rows(model, n_classes, sc, domain, bmax, sr, n, items, lens):
    """One batch of _audio_work on the device -> (WaveformClassifier over the batch's extractor, its rows in ``domain``, lengths)."""
    if lens is None:
        w, lt = A._to_dev(np.stack([x for _, x in items])), None
        ex = A._extractor(int(sr), int(n), min(w.shape[0], model._max_batch))
    else:
        w, lt = _padded_rows(items, n, lens)
        ex = A._extractor(int(sr), int(n), min(w.shape[0], bmax))
    cut = lambda s: None if lt is None else lt[s:s + ex.batch_max]
    clf = A.WaveformClassifier(model, n_classes, extractor=ex, mean=sc.mean_, scale=sc.scale_, domain=domain)
    x = torch.cat([ex.resample(w[s:s + ex.batch_max], n_valid=cut(s)) for s in range(0, w.shape[0], ex.batch_max)]) if domain == "22k" else w
    return clf, x, lt


class _TestRows:
    """What a sweep or read-out runs over, prepared once.  The arguments are refused in one order -- over="audio" without
    ``test_filenames``, then ``domain``, then ``over`` -- before anything touches a device; ``limit`` keeps the first N rows / files;
    standardize="before" standardises (train, val, test) once.  Afterwards: ``train_data`` / ``val_data`` (standardised if "before"),
    ``n`` rows or files, ``what`` ("rows" | "files"), ``x`` (over="mfcc": the float32 NumPy rows) or ``filenames``, ``scaler`` and
    ``bmax`` (over="audio": _audio_work's), and ``batches(model)``."""

    def __init__(self, models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit):
        if over == "audio":
            if test_filenames is None:
                raise ValueError("over='audio' needs test_filenames (test_dataset_to_add_noise/test_filenames.npy)")
            if domain not in ("22k", "input"):
                raise ValueError(f"domain={domain!r}: '22k' or 'input'")
        elif over != "mfcc":
            raise ValueError("over must be 'audio' or 'mfcc'")
        self.over, self.domain, self.limit, self.what = over, domain, limit, "files" if over == "audio" else "rows"
        if standardize == "before":
            train_data, val_data, test_data = A.standardize_dataset(train_data, val_data, test_data)
        self.train_data, self.val_data = train_data, val_data
        if over == "audio":
            self.filenames = list(self.limited(test_filenames))
            self._work, self.scaler, self.bmax = _audio_work(models, train_data, val_data, self.filenames)
            self.n = len(self.filenames)
        else:
            self.x = np.asarray(self.limited(test_data), dtype=np.float32)
            self.n = len(self.x)

    def limited(self, rows):
        """The first ``limit`` of ``rows`` (labels, names: anything that goes row for row with the test set)."""
        return rows[:self.limit] if self.limit else rows

    def classifier(self, model):
        """over="mfcc": the model as the reference wraps it (:500-504)."""
        return A.TensorFlowV2Classifier(model=model, nb_classes=model._n_classes, input_shape=(self.x.shape[1],),
                                        loss_object=CategoricalCrossentropy())

    def batches(self, model):
        """Yields (estimator, x, lengths, idx): ``x`` are the rows ``idx`` of the test set as ``estimator`` takes them.  over="mfcc":
        one batch, every row, as NumPy, no lengths; over="audio": one batch per entry of _audio_work, on the device."""
        if self.over == "mfcc":
            yield self.classifier(model), self.x, None, slice(None)
            return
        for sr, n, items, lens in self._work:
            clf, x, lt = _audio_rows(model, model._n_classes, self.scaler, self.domain, self.bmax, sr, n, items, lens)
            yield clf, x, lt, [i for i, _ in items]


def white_box_sweep(models, train_data, val_data, test_data, test_labels, kind="fgsm", standardize="before", grid=None,
                    points=None, limit=None, over="mfcc", test_filenames=None, domain="22k", **attack_kw):
    """attacks.py:493-693.  The models are wrapped as TensorFlowV2Classifier(model=, nb_classes=, input_shape=,
    loss_object=) (:500-504) and attacked with ART's constructor keywords; JSMA runs on the first 100 test rows (:552).
    kind="apgd" (ours): lipasr.attacks.AutoProjectedGradientDescent on PGD's grid, ``attack_kw`` its keywords.
    kind="auto" (ours): lipasr.attacks.AutoAttack on PGD's grid (the first step size 2 eps, the paper's, unless ``attack_kw`` gives
    eps_step; MFCC rows are SquareAttack's 20 x frames picture, audio rows a strip): the accuracy that survives all its members.
    over="audio" (kind fgsm | pgd | apgd | auto): the attack perturbs the audio of ``test_filenames`` through WaveformClassifier -- the 22 050 Hz
    signal (domain="22k", what the black-box audio noise perturbs) or the file's own samples (domain="input"); eps is an
    amplitude, iterates stay in [-1, 1].  The reference has no such sweep, so the default grid is OURS: AUDIO_SIGMAS, which lays
    the curve over black_box_sweep(over="audio", kind="simple").  Features are standardized with the statistics of (train, val,
    clean test MFCCs), fused into the extraction: the statistics black_box_sweep(over="audio") derives at sigma = 0, so the two
    sweeps agree at strength 0."""
    if over == "audio" and kind not in ("fgsm", "pgd", "apgd", "auto"):
        raise ValueError(f"over='audio' runs kind 'fgsm', 'pgd', 'apgd' and 'auto', not {kind!r} (C&W and JSMA perturb the MFCC vector only)")
    if kind == "fgsm":
        default = np.linspace(1, 30, 50) if standardize == "after" else np.linspace(0.01, 0.3, 10)  # :497-499
        build = lambda clf, item: A.FastGradientMethod(estimator=clf, eps=item, **attack_kw)
    elif kind == "pgd":
        default = np.linspace(1, 30, 50)                                                             # :648
        build = lambda clf, item: A.ProjectedGradientDescent(estimator=clf, eps=item, **attack_kw)
    elif kind == "apgd":  # ours: Auto-PGD (attack_kw: norm, loss_type, max_iter, nb_random_init, ...) on PGD's grid
        default = np.linspace(1, 30, 50)
        build = lambda clf, item: A.AutoProjectedGradientDescent(estimator=clf, eps=item, **attack_kw)
    elif kind == "auto":  # ours: the AutoAttack ensemble (attack_kw: norm, eps_step, attacks, batch_size, seed) on PGD's grid
        default = np.linspace(1, 30, 50)
        build = lambda clf, item: A.AutoAttack(clf, eps=item, **{"eps_step": 2.0 * item, "shape": _picture(clf, over), **attack_kw})
    elif kind == "jsma":
        default, limit = [10], (100 if limit is None else limit)                                     # :539, :552
        build = lambda clf, item: A.SaliencyMapMethod(classifier=clf, theta=item, gamma=0.1, **attack_kw)
    elif kind == "linf":
        default = [10]                                                                               # :572
        build = lambda clf, item: A.CarliniLInfMethod(classifier=clf, confidence=item, **attack_kw)
    elif kind == "l2":
        default = np.linspace(1, 300, 3)                                                             # :607
        build = lambda clf, item: A.CarliniL2Method(classifier=clf, confidence=item, **attack_kw)
    else:
        raise ValueError(f"unknown white-box attack {kind!r}")
    rows = _TestRows(models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit)
    labels = rows.limited(test_labels)
    if over == "audio":
        grid = list(AUDIO_SIGMAS if grid is None else grid)[:points]
        acc = {name: [] for name in models}
        for item in grid:
            for name, model in models.items():
                pred = np.zeros((rows.n, labels.shape[1]))
                for clf, x, lt, idx in rows.batches(model):
                    adv = build(clf, item).generate_device(x, None, lengths=lt) if item != 0 else x
                    pred[idx] = clf.predict_device(adv, lengths=lt).cpu().numpy()
                a = accuracy(pred, labels)
                acc[name].append(a)
                print(f"Accuracy on adversarial audio test examples{_tag(name)}: {a * 100}% ({item})")
        return grid, {k: np.asarray(v) for k, v in acc.items()}
    grid = list(default if grid is None else grid)[:points]
    clfs = {name: rows.classifier(m) for name, m in models.items()}

    def make(name, clf, item):
        adv = build(clf, item).generate(x=rows.x)
        return A.standardize_dataset(rows.train_data, rows.val_data, adv)[2] if standardize == "after" else adv

    return _sweep(clfs, grid, make, labels, "adversarial")


# ours (the reference has no query-only attack): L-inf radii for lipasr.attacks.GeneticAttack.  Over MFCC rows the grid is the
# white-box FGSM one (:497-499), so that the curve lies over white_box_sweep's; over audio a short list of amplitudes out of AUDIO_SIGMAS
GENETIC_AUDIO_EPS = [0.002, 0.004, 0.01, 0.02, 0.05]


def _picture(clf, over):
    """SquareAttack's ``shape`` for the rows of ``clf``: 20 coefficients x frames for MFCC rows, a strip (None) for audio."""
    return (20, clf.input_shape[0] // 20) if over == "mfcc" else None


def _query_sweep(build, what, models, train_data, val_data, test_data, test_labels, over, standardize, test_filenames, domain, grid,
                 points, limit):
    """What genetic_sweep and square_sweep share: ``build(clf, eps)`` makes the attack, which leaves success_ and queries_ behind."""
    rows = _TestRows(models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit)
    labels = rows.limited(test_labels)
    if over == "audio":
        default = GENETIC_AUDIO_EPS
    else:
        default = np.linspace(1, 30, 50) if standardize == "after" else np.linspace(0.01, 0.3, 10)  # white_box_sweep's FGSM grid
    grid = list(default if grid is None else grid)[:points]
    acc, queries = {name: [] for name in models}, {name: [] for name in models}
    for item in grid:
        for name, model in models.items():
            pred = np.zeros((rows.n, labels.shape[1]))
            ok, q = np.zeros(rows.n, dtype=bool), np.zeros(rows.n, dtype=np.int64)
            for clf, x, lt, idx in rows.batches(model):
                atk = build(clf, item)
                if over == "audio":
                    adv = atk.generate_device(x, None, lengths=lt)
                    pred[idx] = clf.predict_device(adv, lengths=lt).cpu().numpy()
                else:  # NumPy rows in and out, standardised where the deployed pipeline does it, classified by the model itself
                    adv = atk.generate(x)
                    if standardize == "after":
                        adv = A.standardize_dataset(rows.train_data, rows.val_data, adv)[2]
                    pred[idx] = model.predict(adv)
                ok[idx], q[idx] = atk.success_.cpu().numpy(), atk.queries_.cpu().numpy()
            a = accuracy(pred, labels)
            mean_q = float(np.mean(q[ok])) if ok.any() else float("nan")
            acc[name].append(a)
            queries[name].append(mean_q)
            print(f"Accuracy on {what} black-box {'audio ' if over == 'audio' else ''}test examples{_tag(name)}: {a * 100}% ({item}); "
                  f"{int(ok.sum())} of {len(ok)} clips succeeded, mean queries of those: {mean_q}")
    return grid, {k: np.asarray(v) for k, v in acc.items()}, {k: np.asarray(v) for k, v in queries.items()}


def genetic_sweep(models, train_data, val_data, test_data, test_labels, over="mfcc", standardize="before", test_filenames=None,
                  domain="22k", grid=None, points=None, limit=None, **attack_kw):
    """The genetic black-box attack (lipasr.attacks.GeneticAttack: scores only, no gradient) against its L-inf radius eps, untargeted,
    from each model's own predictions: per model and eps the accuracy on the attacked rows and the mean number of queries the
    successful clips took.  over="mfcc": the rows of ``test_data`` (standardize as in white_box_sweep; the default grid is its FGSM
    grid); over="audio": the audio of ``test_filenames`` through WaveformClassifier, prepared as in white_box_sweep(over="audio")
    (default grid GENETIC_AUDIO_EPS, amplitudes; iterates stay in [-1, 1]).  ``attack_kw``: GeneticAttack's keywords (pop_size,
    max_iter, mutation_p, ...).  A query-only attack that ends BELOW the gradient attacks' accuracy at the same eps says that the
    gradients are masked.  Returns (grid, {model name: accuracies}, {model name: mean queries of the successful clips, nan if none})."""
    return _query_sweep(lambda clf, item: A.GeneticAttack(clf, item, **attack_kw), "genetic", models, train_data, val_data, test_data,
                        test_labels, over, standardize, test_filenames, domain, grid, points, limit)


def square_sweep(models, train_data, val_data, test_data, test_labels, over="mfcc", standardize="before", test_filenames=None,
                 domain="22k", grid=None, points=None, limit=None, **attack_kw):
    """Square Attack (lipasr.attacks.SquareAttack: one score query per iteration, no gradient) against its L-inf radius eps, as
    genetic_sweep runs GeneticAttack: the same rows, the same grids, the same return triple with the mean queries of the successful
    clips.  MFCC rows are 20 x frames pictures, audio rows strips with their lengths.  ``attack_kw``: SquareAttack's keywords
    (max_iter, p_init, nb_restarts, ...)."""
    return _query_sweep(lambda clf, item: A.SquareAttack(clf, eps=item, **{"shape": _picture(clf, over), **attack_kw}), "square", models,
                        train_data, val_data, test_data, test_labels, over, standardize, test_filenames, domain, grid, points, limit)


def time_warp_sweep(models, train_data, val_data, test_data, test_labels, test_filenames, max_rate=1.0, max_gain_db=0.0,
                    counts=(9, 3, 3), refine_steps=0, rooms=None, room_taps=2048, room_t60=(0.15, 0.5), room_seed=0, domain="22k",
                    standardize="before", grid=None, points=None, limit=None):
    """The time-warp attack (lipasr.attacks.TimeWarp: the worst of a grid of delays, speeds and levels per clip; refine_steps > 0
    adds its first-order steps) against the largest delay either way, ``grid`` in MILLISECONDS (default WARP_SHIFTS_MS), with
    ``max_rate``, ``max_gain_db`` and ``counts`` held fixed: per model and delay one accuracy line.  Audio only -- files, lengths
    and standardisation as in white_box_sweep(over="audio"); the labels are the true ones, so a clip that is wrong when clean
    counts as wrong at every delay.  A triple found inside a smaller box lies inside every larger one, so a clip's margin at a
    delay is the smallest found at any delay of the grid up to it: the accuracies cannot rise with the delay.  ``rooms``: the
    attack and the read-out run through a bank of that many synthetic rooms (OverTheAirClassifier).  An axis whose box has no
    width (a delay of 0, max_rate 1, max_gain_db 0) is searched with one candidate, not ``counts`` copies of it.
    Returns (grid, {model name: accuracies})."""
    rows = _TestRows(models, train_data, val_data, test_data, "audio", standardize, test_filenames, domain, limit)
    truth = np.asarray(rows.limited(test_labels)).argmax(axis=1)
    grid = [float(d) for d in list(WARP_SHIFTS_MS if grid is None else grid)[:points]]
    if any(d < 0 for d in grid):
        raise ValueError(f"delays in milliseconds, not negative: {grid}")
    banks = {}

    def through(clf, rate):
        if rooms is None:
            return clf
        from .room import RoomChannel, synthetic_rirs

        if rate not in banks:
            banks[rate] = RoomChannel(synthetic_rirs(int(rooms), sr=rate, taps=room_taps, t60=room_t60, seed=room_seed))
        return A.OverTheAirClassifier(clf, banks[rate])

    acc = {name: [] for name in models}
    for name, model in models.items():
        margins = np.full((len(grid), rows.n), np.inf)
        for (sr, _, _, _), (clf, x, lt, idx) in zip(rows._work, rows.batches(model)):
            rate = 22050 if domain == "22k" else int(sr)
            est = through(clf, rate)
            y = torch.as_tensor(truth[idx])
            for k, ms in enumerate(grid):
                used = tuple(c if wide else 1 for c, wide in zip(counts, (ms > 0, max_rate > 1.0, max_gain_db > 0.0)))
                atk = A.TimeWarp(est, max_shift=ms * 1e-3 * rate, max_rate=max_rate, max_gain_db=max_gain_db, counts=used,
                                 refine_steps=refine_steps)
                atk.generate_device(x, y, lengths=lt)
                margins[k, idx] = atk.margins_.cpu().numpy()
        for k, ms in enumerate(grid):
            found = margins[[j for j, other in enumerate(grid) if other <= ms]].min(axis=0)
            a = float(np.mean(found > 0)) if rows.n else float("nan")
            acc[name].append(a)
            print(f"Accuracy on time-warped audio test examples{_tag(name)}: {a * 100}% ({ms} ms)")
    return grid, {k: np.asarray(v) for k, v in acc.items()}


def hopskipjump_sweep(models, train_data, val_data, test_data, test_labels, over="mfcc", standardize="before", test_filenames=None,
                      domain="22k", norm=np.inf, grid=None, points=None, limit=None, **attack_kw):
    """HopSkipJump (lipasr.attacks.HopSkipJump: the label only, neither score nor gradient) -- ONE run per model, not one per eps: the
    attack minimises the distance, and from its ``distance_`` per clip comes the whole curve.  The labels are the true ones, so a
    row that is wrong when clean has distance 0; accuracy at eps is the share of rows with distance_ > eps (an upper bound on the
    robust accuracy, as every attack gives), at the points of white_box_sweep's PGD grid (over="audio": AUDIO_SIGMAS, its grid
    there).  ``norm``: 2 or np.inf, the norm of the distance and of eps; ``attack_kw``: HopSkipJump's keywords (max_iter, max_eval,
    ...).  Rows are prepared as in square_sweep; standardize="after" is refused (the distance would be one between unstandardised
    rows that the models never see).  Returns (grid, {model name: accuracies}, {model name: {"median_distance": over the rows with
    a finite distance, "mean_queries": over all rows}})."""
    if norm not in (2, 2.0, np.inf):
        raise ValueError(f"norm = {norm!r}: HopSkipJump runs in norm 2 or inf")
    if standardize != "before":
        raise ValueError("hopskipjump_sweep measures distances between the rows the models see: standardize='before'")
    rows = _TestRows(models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit)
    labels = np.asarray(rows.limited(test_labels))
    grid = list((AUDIO_SIGMAS if over == "audio" else np.linspace(1, 30, 50)) if grid is None else grid)[:points]
    acc, stats = {}, {}
    for name, model in models.items():
        dist, q = np.zeros(rows.n, dtype=np.float64), np.zeros(rows.n, dtype=np.int64)
        for clf, x, lt, idx in rows.batches(model):
            atk = A.HopSkipJump(clf, norm=norm, **{"verbose": False, **attack_kw})
            y = torch.as_tensor(labels[idx])
            if over == "audio":
                atk.generate_device(x, y, lengths=lt)
            else:
                atk.generate(x, y)
            dist[idx], q[idx] = atk.distance_.cpu().numpy(), atk.queries_.cpu().numpy()
        acc[name] = np.asarray([float(np.mean(dist > eps)) if rows.n else float("nan") for eps in grid])
        finite = dist[np.isfinite(dist)]
        stats[name] = {"median_distance": float(np.median(finite)) if len(finite) else float("nan"),
                       "mean_queries": float(np.mean(q)) if rows.n else float("nan")}
        what = f"HopSkipJump (norm {'inf' if norm == np.inf else 2}) black-box {'audio ' if over == 'audio' else ''}test examples{_tag(name)}"
        for eps, a in zip(grid, acc[name]):
            print(f"Accuracy on {what}: {a * 100}% ({eps})")
        print(f"{what}: median distance {stats[name]['median_distance']}, mean queries {stats[name]['mean_queries']} over {rows.n} {rows.what}")
    return grid, acc, stats


OVER_THE_AIR_KINDS = ("fgsm", "pgd", "apgd", "auto", "genetic", "square")


def _radius_attacks(attack_kw):
    """kind -> build(estimator over audio, eps): the attacks of OVER_THE_AIR_KINDS with ``attack_kw`` as their keywords."""
    return {"fgsm": lambda clf, e: A.FastGradientMethod(estimator=clf, eps=e, **attack_kw),
            "pgd": lambda clf, e: A.ProjectedGradientDescent(estimator=clf, eps=e, **attack_kw),
            "apgd": lambda clf, e: A.AutoProjectedGradientDescent(estimator=clf, eps=e, **attack_kw),
            "auto": lambda clf, e: A.AutoAttack(clf, eps=e, **{"eps_step": 2.0 * e, "shape": None, **attack_kw}),
            "genetic": lambda clf, e: A.GeneticAttack(clf, e, **attack_kw),
            "square": lambda clf, e: A.SquareAttack(clf, eps=e, **{"shape": None, **attack_kw})}


def over_the_air_sweep(models, train_data, val_data, test_data, test_labels, test_filenames, kind="pgd", rooms=4, room_taps=2048,
                       room_t60=(0.15, 0.5), room_seed=0, domain="22k", standardize="before", grid=None, points=None, limit=None,
                       **attack_kw):
    """What is left of an attack over audio once it is PLAYED: two disjoint banks of ``rooms`` synthetic room impulse responses
    each (lipasr.room.synthetic_rirs, one draw of 2 x rooms split in halves: an attack bank A and a held-out bank B), and per model
    and grid point three accuracies, each the share of (clip, room of B) pairs the model still gets right:
        "clean"   the clean clips through B
        "dry"     adversarial clips made without the room (the attack of white_box_sweep / the query sweeps) through B
        "air"     adversarial clips made through A (the same attack over OverTheAirClassifier: expectation over A) through B
    ``kind``: one of OVER_THE_AIR_KINDS -- the attacks that optimise within a radius eps; the labels they push away from are each
    model's own on the dry clip.  Files, lengths and standardisation as in white_box_sweep(over="audio"); the default grid is
    AUDIO_SIGMAS for the gradient attacks and GENETIC_AUDIO_EPS for the query attacks.  The responses are drawn at the rate of the
    rows (22 050 Hz for domain="22k").  Returns (grid, {model name: {"clean" | "dry" | "air": accuracies}})."""
    from .room import RoomChannel, synthetic_rirs

    builders = _radius_attacks(attack_kw)
    if kind not in builders:
        raise ValueError(f"a room takes an attack that optimises within a radius -- {', '.join(OVER_THE_AIR_KINDS)} -- not {kind!r}")
    rooms = int(rooms)
    if rooms < 1:
        raise ValueError(f"rooms = {rooms}: at least one room per bank")
    rows = _TestRows(models, train_data, val_data, test_data, "audio", standardize, test_filenames, domain, limit)
    truth = np.asarray(rows.limited(test_labels)).argmax(axis=1)
    grid = list((GENETIC_AUDIO_EPS if kind in ("genetic", "square") else AUDIO_SIGMAS) if grid is None else grid)[:points]
    banks = {}  # rate of the rows -> (A, B)

    def channels(rate):
        if rate not in banks:
            h = synthetic_rirs(2 * rooms, sr=rate, taps=room_taps, t60=room_t60, seed=room_seed)
            banks[rate] = (RoomChannel(h[:rooms]), RoomChannel(h[rooms:]))
        return banks[rate]

    acc = {name: {k: [] for k in ("clean", "dry", "air")} for name in models}
    for item in grid:
        for name, model in models.items():
            hits = {k: np.zeros((rows.n, rooms), dtype=bool) for k in ("clean", "dry", "air")}
            for (sr, _, _, _), (clf, x, lt, idx) in zip(rows._work, rows.batches(model)):
                bank_a, bank_b = channels(22050 if domain == "22k" else int(sr))
                through_a, through_b = A.OverTheAirClassifier(clf, bank_a), A.OverTheAirClassifier(clf, bank_b)
                made = {"clean": x,
                        "dry": build_or_keep(builders[kind], clf, item, x, lt),
                        "air": build_or_keep(builders[kind], through_a, item, x, lt)}
                for k, rows_k in made.items():
                    heard = through_b.predict_each_device(rows_k, lengths=lt, logits=True).argmax(dim=2).cpu().numpy()
                    hits[k][idx] = heard == truth[idx][:, None]
            for k, label in (("clean", "clean audio"), ("dry", "adversarial audio made without the room"),
                             ("air", "adversarial audio made through the attack rooms")):
                a = float(hits[k].mean()) if rows.n else float("nan")
                acc[name][k].append(a)
                print(f"Accuracy through {rooms} held-out rooms on {label}{_tag(name)}: {a * 100}% ({item})")
    return grid, {name: {k: np.asarray(v) for k, v in d.items()} for name, d in acc.items()}


def defended_sweep(models, train_data, val_data, test_data, test_labels, test_filenames, defence, kind="pgd", backward="chain",
                   detect_fpr=0.05, domain="22k", standardize="before", grid=None, points=None, limit=None, **attack_kw):
    """An input-transformation defence under attack (lipasr.defences, estimators.DefendedClassifier).  ``defence``: the text form
    lipasr.defences.parse_defence takes, e.g. "median:5,lowpass:4000:101,quantize:8"; its taps are designed at the rate of the rows
    (22 050 Hz for domain="22k").  Per model and grid point four numbers:
        "undefended"  accuracy of the model on adversarial clips made against it
        "static"      accuracy of the DEFENDED model on those same clips: the attacker does not know of the defence
        "adaptive"    accuracy of the defended model on clips made against itself: the attacker differentiates through the defence
                      (backward="chain") or takes it as the identity on the way back (backward="identity", BPDA); a query attack
                      simply queries the defended model
        "detected"    the share of the static clips that lipasr.defences.TransformationDetector flags at the false-positive rate
                      ``detect_fpr``.  The threshold is fitted on the clean FIRST half of every batch of files (the split
                      universal_sweep makes), and the flagged share is that of the static clips of the SECOND halves.
    ``kind``: one of OVER_THE_AIR_KINDS; the labels the attacks push away from are each estimator's own.  Files, lengths,
    standardisation and default grids as in over_the_air_sweep.  Returns (grid, {model name: {the four names: values per point}})."""
    from .defences import AudioDefence, TransformationDetector, parse_defence

    builders = _radius_attacks(attack_kw)
    if kind not in builders:
        raise ValueError(f"a defence is put under an attack that optimises within a radius -- {', '.join(OVER_THE_AIR_KINDS)} -- not {kind!r}")
    if backward not in ("chain", "identity"):
        raise ValueError(f"backward={backward!r}: 'chain' or 'identity'")
    if not 0.0 <= float(detect_fpr) <= 1.0:
        raise ValueError(f"detect_fpr = {detect_fpr}: a share in [0, 1]")
    parse_defence(defence, 22050)  # a wrong text is refused before anything touches a device
    rows = _TestRows(models, train_data, val_data, test_data, "audio", standardize, test_filenames, domain, limit)
    labels = rows.limited(test_labels)
    truth = np.asarray(labels).argmax(axis=1)
    grid = list((GENETIC_AUDIO_EPS if kind in ("genetic", "square") else AUDIO_SIGMAS) if grid is None else grid)[:points]
    chains = {}  # rate of the rows -> AudioDefence

    def chain(rate):
        if rate not in chains:
            chains[rate] = AudioDefence(parse_defence(defence, rate))
        return chains[rate]

    keys = ("undefended", "static", "adaptive", "detected")
    acc = {name: {k: [] for k in keys} for name in models}
    for item in grid:
        for name, model in models.items():
            hits = {k: np.zeros(rows.n, dtype=bool) for k in keys[:3]}
            clean_scores, static_scores = [], []
            for (sr, _, _, _), (clf, x, lt, idx) in zip(rows._work, rows.batches(model)):
                d = chain(22050 if domain == "22k" else int(sr))
                defended = A.DefendedClassifier(clf, d, backward=backward)
                static = build_or_keep(builders[kind], clf, item, x, lt)
                adaptive = build_or_keep(builders[kind], defended, item, x, lt)
                for k, est, rows_k in (("undefended", clf, static), ("static", defended, static), ("adaptive", defended, adaptive)):
                    hits[k][idx] = est.predict_device(rows_k, lengths=lt, logits=True).argmax(dim=1).cpu().numpy() == truth[idx]
                half = x.shape[0] // 2
                cut = lambda t, s: None if t is None else t[s]
                det = TransformationDetector(clf, [d])
                clean_scores.append(det.scores(x[:half].contiguous(), cut(lt, slice(0, half))).cpu().numpy())
                static_scores.append(det.scores(static[half:].contiguous(), cut(lt, slice(half, None))).cpu().numpy())
            clean_scores, static_scores = np.concatenate(clean_scores), np.concatenate(static_scores)
            if len(clean_scores) and len(static_scores):
                det.fit_scores(clean_scores, detect_fpr)
                threshold, rate = det.threshold, float(np.mean(det.flag_scores(static_scores)))
            else:
                threshold = rate = float("nan")
            for k, label in (("undefended", "Accuracy of the undefended model on adversarial audio"),
                             ("static", "Accuracy of the defended model on adversarial audio made against the undefended one (static)"),
                             ("adaptive", f"Accuracy of the defended model on adversarial audio made against itself (adaptive, backward {backward})")):
                a = float(hits[k].mean()) if rows.n else float("nan")
                acc[name][k].append(a)
                print(f"{label}{_tag(name)}: {a * 100}% ({item})")
            acc[name]["detected"].append(rate)
            print(f"Detector hit rate on the static adversarial audio at false-positive rate {detect_fpr}{_tag(name)}: {rate * 100}% ({item}); "
                  f"threshold {threshold} from {len(clean_scores)} clean clips, {len(static_scores)} adversarial clips scored")
    return grid, {name: {k: np.asarray(v) for k, v in d.items()} for name, d in acc.items()}


def universal_sweep(models, train_data, val_data, test_data, test_labels, over="mfcc", standardize="before", test_filenames=None,
                    domain="22k", norm=np.inf, rooms=None, room_taps=2048, room_t60=(0.15, 0.5), room_seed=0, grid=None, points=None,
                    limit=None, **attack_kw):
    """ONE perturbation for every clip (lipasr.attacks.UniversalPerturbation) against its radius eps.  Per model and eps the noise
    is FITTED on the first half of the test rows (over="audio": of every batch of files that share a rate and a row length, since a
    noise vector has one period) from the model's own predictions, and the accuracy is that of the SECOND half with that noise
    added -- rows the fit never saw: the generalisation that makes the perturbation universal.  Next to it: the fooling rate on the
    fitting half.  Rows, standardisation (standardize="before" only: the noise lives on the rows the models see) and grids as in
    white_box_sweep: its FGSM grid (norm inf) or PGD grid (norm 2) over MFCC rows, AUDIO_SIGMAS without the 0 over audio.
    ``rooms`` (over="audio"): the fit runs through a bank of that many synthetic rooms (OverTheAirClassifier) and the held-out
    half is heard through a disjoint bank, as over_the_air_sweep does.  ``attack_kw``: UniversalPerturbation's keywords (max_iter,
    length, random_shift, eps_step, delta, ...).  Returns (grid, {model name: held-out accuracies}, {model name: fooling rates
    of the fitting half})."""
    if norm not in (2, 2.0, np.inf):
        raise ValueError(f"norm = {norm!r}: UniversalPerturbation runs in norm 2 or inf")
    if standardize != "before":
        raise ValueError("universal_sweep fits the noise on the rows the models see: standardize='before'")
    if rooms is not None and over != "audio":
        raise ValueError("rooms= goes with over='audio'")
    rows = _TestRows(models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit)
    truth = np.asarray(rows.limited(test_labels)).argmax(axis=1)
    if over == "audio":
        default = AUDIO_SIGMAS[1:]
    else:
        default = np.linspace(0.01, 0.3, 10) if norm == np.inf else np.linspace(1, 30, 50)
    grid = list(default if grid is None else grid)[:points]
    banks = {}

    def through(clf, sr):
        """(the estimator the noise is fitted over, the one the held-out rows are heard through)"""
        if rooms is None:
            return clf, clf
        from .room import RoomChannel, synthetic_rirs

        rate = 22050 if domain == "22k" else int(sr)
        if rate not in banks:
            h = synthetic_rirs(2 * int(rooms), sr=rate, taps=room_taps, t60=room_t60, seed=room_seed)
            banks[rate] = (RoomChannel(h[:int(rooms)]), RoomChannel(h[int(rooms):]))
        return A.OverTheAirClassifier(clf, banks[rate][0]), A.OverTheAirClassifier(clf, banks[rate][1])

    acc, fooled = {name: [] for name in models}, {name: [] for name in models}
    for item in grid:
        for name, model in models.items():
            hits, seen, rate_sum, fitted = 0, 0, 0.0, 0
            rates = [sr for sr, _, _, _ in rows._work] if over == "audio" else [None]
            for sr, (clf, x, lt, idx) in zip(rates, rows.batches(model)):
                xt = clf.rows_device(x)
                half = xt.shape[0] // 2
                if half == 0:
                    continue
                idx = np.arange(rows.n)[idx]
                cut = lambda t, s: None if t is None else t[s]
                fit_clf, hear_clf = through(clf, sr)
                atk = A.UniversalPerturbation(fit_clf, eps=item, norm=norm, **attack_kw)
                atk.generate_device(xt[:half].contiguous(), None, lengths=cut(lt, slice(0, half)))
                held = atk.apply(xt[half:].contiguous(), lengths=cut(lt, slice(half, None)))
                pred = hear_clf.predict_device(held, logits=True, lengths=cut(lt, slice(half, None))).argmax(dim=1).cpu().numpy()
                hits += int((pred == truth[idx[half:]]).sum())
                seen += len(pred)
                rate_sum += atk.fooling_rate * half
                fitted += half
            a = hits / seen if seen else float("nan")
            f = rate_sum / fitted if fitted else float("nan")
            acc[name].append(a)
            fooled[name].append(f)
            print(f"Accuracy on held-out {'audio ' if over == 'audio' else ''}test examples under a universal perturbation{_tag(name)}: "
                  f"{a * 100}% ({item}); fooling rate on the {fitted} fitting {rows.what}: {f * 100}%")
    return grid, {k: np.asarray(v) for k, v in acc.items()}, {k: np.asarray(v) for k, v in fooled.items()}


def build_or_keep(build, clf, item, x, lt):
    """The attack ``build(clf, item)`` on the rows ``x``, or the rows themselves at strength 0."""
    return build(clf, item).generate_device(x, None, lengths=lt) if item != 0 else x


def dolphin_sweep(models, train_data, val_data, test_data, test_labels, test_filenames, grid=DOLPHIN_CARRIER_LEVELS, a1=1.0, a2=0.5,
                  standardize="before", points=None, limit=None):
    """DolphinAttack (lipasr.dolphin) against the carrier level: every file of ``test_filenames`` (16 kHz) becomes amplitude-
    modulated ultrasound on a 30 kHz carrier, a microphone with the non-linearity a1 s + a2 s^2 records it
    (DolphinAttack.generate_recorded: the 192 kHz signal never reaches memory), and the recorded 16 kHz clip goes through the
    MFCC extractor with the file's own length.  Features are standardized with the statistics of (train, val, clean test MFCCs),
    as in white_box_sweep(over="audio").  Accuracy is against the command's OWN label: a high value means that the inaudible
    command was understood.  A grid item of None stands for no attack (the file itself through the same extraction): there the
    sweep agrees with black_box_sweep(over="audio") at sigma 0.  Returns (grid, {model name: accuracies})."""
    from .dolphin import DolphinAttack

    if test_filenames is None:
        raise ValueError("dolphin_sweep needs test_filenames (test_dataset_to_add_noise/test_filenames.npy)")
    test_filenames = list(test_filenames[:limit] if limit else test_filenames)
    labels = test_labels[:limit] if limit else test_labels
    clips = []
    for fn in test_filenames:
        x, sr = A.read_wav(fn)
        if sr != 16000:
            raise ValueError(f"{fn}: {sr} Hz; the DolphinAttack chain takes 16 kHz files")
        clips.append(x)
    if standardize == "before":
        train_data, val_data, _ = A.standardize_dataset(train_data, val_data, test_data)
    grid = list(grid)[:points]
    lens = np.array([len(x) for x in clips], dtype=np.int32)
    same = bool(np.all(lens == lens[0]))
    # one length: rows as they are, extraction as black_box_sweep(over="audio") runs it; several: rows padded to the longest clip
    # rounded up to a multiple of 4000 samples (compute_mfcc_all_files' rule), each clip with its own length
    n_pad = int(lens[0]) if same else -(-int(lens.max()) // 4000) * 4000
    w, lt = _padded_rows(list(enumerate(clips)), n_pad, lens)
    lt = None if same else lt
    bmax = min(w.shape[0], 256)
    ex = A._extractor(16000, n_pad, bmax)

    def features(rows):
        out = []
        for s in range(0, rows.shape[0], ex.batch_max):
            r = rows[s:s + ex.batch_max]
            out.append(ex.from_22k(ex.resample(r), 44) if lt is None else ex(r, 44, n_valid=lt[s:s + ex.batch_max]))
        return torch.cat(out)

    clean = features(w)
    sc = A.StandardScaler().fit(torch.cat([A._to_dev(train_data), A._to_dev(val_data), clean]))
    acc = {name: [] for name in models}
    for item in grid:
        if item is None:
            feats = clean
        else:
            da = DolphinAttack(16000, n_pad, bmax, carrier_level=float(item))
            rec = torch.cat([da.generate_recorded(w[s:s + bmax], None if lt is None else lt[s:s + bmax], a1=a1, a2=a2)
                             for s in range(0, w.shape[0], bmax)])
            da.close()
            feats = features(rec)
        x = sc.transform_device(feats).cpu().numpy()
        for name, model in models.items():
            a = accuracy(model.predict(x), labels)
            acc[name].append(a)
            print(f"Accuracy on DolphinAttack recordings{_tag(name)}: {a * 100}% (carrier level {item})")
    return grid, {k: np.asarray(v) for k, v in acc.items()}


def imperceptible_report(models, train_data, val_data, test_data, test_labels, test_filenames, eps, learning_rate_1, learning_rate_2,
                         domain="22k", standardize="before", limit=None, seed=0, **attack_kw):
    """ImperceptibleASR (lipasr.attacks) over the audio of ``test_filenames``, targets from random_targets(test_labels): per model
    the targeted success rate, the mean masking loss L_theta after stage 1 and after stage 2 -- how far the perturbation's spectrum
    stands above what the clip itself masks -- and the mean perturbation SNR in dB.  Files are grouped by (rate, length); features
    are standardised as white_box_sweep(over="audio") does.  ``eps`` and the learning rates are amplitudes and have no defaults.
    Returns {model name: {"success", "loss_theta_1", "loss_theta_2", "snr_db", "rows": per-file arrays}}."""
    prep = _TestRows(models, train_data, val_data, test_data, "audio", standardize, test_filenames, domain, limit)
    labels = np.asarray(prep.limited(test_labels))
    n_classes = labels.shape[1]
    targets = A.random_targets(labels, n_classes, rng=np.random.RandomState(seed)).astype(np.float32)
    groups = A._files_to_batches(prep.filenames)  # by (rate, length) and without lengths: the masker takes clips of one length
    out = {}
    for name, model in models.items():
        rows = {k: np.zeros(prep.n) for k in ("success", "loss_theta_1", "loss_theta_2", "snr_db")}
        for (sr, n), items in groups.items():
            clf, x, _ = _audio_rows(model, n_classes, prep.scaler, domain, prep.bmax, sr, n, items, None)
            idx = [i for i, _ in items]
            atk = A.ImperceptibleASR(clf, eps=eps, learning_rate_1=learning_rate_1, learning_rate_2=learning_rate_2, **attack_kw)
            adv = atk.generate_device(x, A._to_dev(targets[idx]))
            atk.masker.close()
            hit = clf.predict_device(adv, logits=True).argmax(dim=1).cpu().numpy() == targets[idx].argmax(axis=1)
            noise = (adv - x).double().pow(2).sum(dim=1)
            snr = 10.0 * torch.log10(x.double().pow(2).sum(dim=1) / noise)
            rows["success"][idx], rows["snr_db"][idx] = hit, snr.cpu().numpy()
            rows["loss_theta_1"][idx], rows["loss_theta_2"][idx] = atk.last_loss_theta_1, atk.last_loss_theta
        r = {k: float(np.mean(v[np.isfinite(v)])) if np.isfinite(v).any() else float("nan") for k, v in rows.items()}
        r["rows"] = rows
        out[name] = r
        tag = _tag(name)
        print(f"Targeted success rate of the imperceptible attack{tag}: {r['success'] * 100}% over {prep.n} files")
        print(f"Mean masking loss L_theta{tag}: {r['loss_theta_1']} after stage 1, {r['loss_theta_2']} after stage 2")
        print(f"Mean perturbation SNR{tag}: {r['snr_db']} dB")
    return out


def lipschitz_report(models, train_data, val_data, test_data, over="mfcc", standardize="before", test_filenames=None, domain="22k",
                     limit=None):
    """Per model: the reference's global read-outs -- get_upper_lipschitz(get_norms(model)) and get_lipschitz_constrained(model) --
    next to what the model does at the test rows: max / mean / median of the local Lipschitz constant of its logits
    (get_local_lipschitz).  over="mfcc": with respect to the MFCC rows of ``test_data``, taken where white_box_sweep attacks them:
    standardised first with standardize="before"; with standardize="after" the rows as they are, which is the point that sweep
    perturbs but NOT an input the deployed pipeline feeds the model (it standardises afterwards), so that figure describes the
    sweep's setting, not the pipeline;
    over="audio": with respect to the audio of ``test_filenames``, the 22 050 Hz signal (domain="22k") or the file's own samples
    (domain="input"), files grouped and features standardised as white_box_sweep(over="audio") does.  limit: the first N rows /
    files.  Returns {model name: {"upper", "constrained", "max", "mean", "median", "local": the per-row float64 array}}."""
    rows = _TestRows(models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit)
    out = {}
    for name, model in models.items():
        local = np.zeros(rows.n)
        for clf, x, lt, idx in rows.batches(model):
            local[idx] = get_local_lipschitz(clf, x, lengths=lt)
        r = {"upper": float(get_upper_lipschitz(get_norms(model))), "constrained": float(get_lipschitz_constrained(model)),
             "max": float(local.max()), "mean": float(local.mean()), "median": float(np.median(local)), "local": local}
        out[name] = r
        tag = _tag(name)
        print(f"Upper Lipschitz bound{tag}: {r['upper']}")
        print(f"Lipschitz constant with the BatchNorm correction{tag}: {r['constrained']}")
        print(f"Local Lipschitz constant over {len(local)} test {rows.what}{tag}: "
              f"max {r['max']} mean {r['mean']} median {r['median']}")
    return out


def radius_report(models, train_data, val_data, test_data, over="mfcc", standardize="before", test_filenames=None, domain="22k",
                  norm=2, limit=None, found_by="deepfool", bounds=None, **attack_kw):
    """Per model: how far the test rows are from the decision boundary (get_robustness_radius) -- the quartiles of the certified
    radius (rows of MFCC features and norm 2 only), of the distance to the linearised boundary and of the distance DeepFool found,
    and the share of rows it flipped.  ``over``, ``standardize``, ``test_filenames``, ``domain`` and ``limit`` as in
    lipschitz_report; ``norm``: 2 or np.inf; attack_kw go to attacks.DeepFool.  found_by="hopskipjump": the found distance and
    the flipped share are attacks.HopSkipJump's, which sees the label only, and attack_kw are its keywords.
    ``bounds``: None, or get_robustness_radius's dict(eps_max=, steps=, method=): only then is "bound_radius" (bound propagation,
    rows of MFCC features, in ``norm``) computed, returned and printed.
    Returns {model name: {"bound": get_lipschitz_bound(model), "margin", "certified" (or None), "linear", "found", "flipped": the
    per-row arrays, "quartiles": {name: (q25, q50, q75)}, "flipped_share"}}."""
    rows = _TestRows(models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit)
    keys = ("margin", "certified", "linear", "found", "flipped") + (("bound_radius",) if bounds is not None else ())
    out = {}
    for name, model in models.items():
        r = {k: np.zeros(rows.n, dtype=bool if k == "flipped" else np.float64) for k in keys}
        for clf, x, lt, idx in rows.batches(model):
            part = get_robustness_radius(clf, x, norm=norm, lengths=lt, found_by=found_by, **({} if bounds is None else {"bounds": bounds}),
                                         **attack_kw)
            for k in keys:
                if part[k] is None:  # no certified radius over audio, nor in norm inf
                    r[k] = None
                else:
                    r[k][idx] = part[k]
        r["bound"] = float(get_lipschitz_bound(model))
        r["quartiles"] = {k: tuple(float(q) for q in np.percentile(r[k], (25, 50, 75))) for k in ("certified", "bound_radius", "linear", "found")
                          if r.get(k) is not None and len(r[k])}
        r["flipped_share"] = float(np.mean(r["flipped"])) if len(r["flipped"]) else float("nan")
        out[name] = r
        tag = _tag(name)
        what = f"{len(r['found'])} test {rows.what}"
        print(f"Lipschitz bound of the logits{tag}: {r['bound']}")
        for k, label in (("certified", "Certified radius"), ("linear", "Distance to the linearised boundary"), ("found", "Distance HopSkipJump found" if found_by == "hopskipjump" else "Distance DeepFool found")):
            if k in r["quartiles"]:
                q = r["quartiles"][k]
                print(f"{label} over {what}{tag}: quartiles {q[0]} {q[1]} {q[2]}")
            else:
                print(f"{label} over {what}{tag}: not given")
        if "bound_radius" in r["quartiles"]:
            q = r["quartiles"]["bound_radius"]
            print(f"Radius certified by bound propagation over {what}{tag}: quartiles {q[0]} {q[1]} {q[2]}")
        print(f"Share of {what} {'HopSkipJump' if found_by == 'hopskipjump' else 'DeepFool'} moved to another class{tag}: {r['flipped_share'] * 100}%")
    return out


def certify_report(models, train_data, val_data, test_data, test_labels, norm=np.inf, method="crown-ibp", standardize="before",
                   grid=None, points=None, limit=None, eps_max=None, steps=12):
    """Bound propagation (lipasr.bounds: IBP / CROWN-IBP) per model over the MFCC test rows: the certified accuracy -- the share of
    rows classified as their label that NO perturbation within eps (in ``norm``: np.inf or 2) moves to another class -- at every
    eps of the PGD sweep's grid (white_box_sweep(kind="pgd"); ``grid`` / ``points`` as there), which stands UNDER the accuracy any
    attack leaves at that eps; the median certified radius of a bisection on [0, eps_max] (default: the grid's largest eps); and,
    for norm 2, the median radius the Lipschitz bound certifies, next to it.  It certifies the base classifier, deterministically.
    Returns {model name: {"grid", "certified_accuracy" (one per eps), "bound_radius" (per row), "lipschitz_median" (or None)}}."""
    from .bounds import certified_accuracy, certified_radius

    rows = _TestRows(models, train_data, val_data, test_data, "mfcc", standardize, None, "22k", limit)
    labels = np.asarray(rows.limited(test_labels)).argmax(axis=1)
    grid = [float(e) for e in list(np.linspace(1, 30, 50) if grid is None else grid)[:points]]
    top = float(max(grid)) if eps_max is None else float(eps_max)
    out = {}
    for name, model in models.items():
        clf = rows.classifier(model)
        r = {"grid": np.asarray(grid), "certified_accuracy": certified_accuracy(clf, rows.x, labels, grid, norm=norm, method=method),
             "bound_radius": certified_radius(clf, rows.x, norm=norm, eps_max=top, steps=steps, method=method).double().cpu().numpy(),
             "lipschitz_median": None}
        if norm == 2 and rows.n and model._n_classes > 1:
            z = torch.topk(model.predict_device(A._to_dev(rows.x), logits=True).double(), 2, dim=1).values
            r["lipschitz_median"] = float(np.median((z[:, 0] - z[:, 1]).cpu().numpy() / (np.sqrt(2.0) * get_lipschitz_bound(model))))
        out[name] = r
        tag = _tag(name)
        what = f"{rows.n} test rows"
        nn = "inf" if norm == np.inf else "2"
        for e, a in zip(grid, r["certified_accuracy"]):
            print(f"Certified accuracy ({method}, norm {nn}) over {what}{tag} at eps {e}: {a * 100}%")
        print(f"Median radius certified by bound propagation over {what}{tag}: {float(np.median(r['bound_radius'])) if rows.n else float('nan')}")
        if r["lipschitz_median"] is not None:
            print(f"Median radius the Lipschitz bound certifies over {what}{tag}: {r['lipschitz_median']}")
    return out


SMOOTH_RADII = (0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)  # in units of sigma: CERTIFY's radius tops out at sigma Phi^-1(alpha^(1/n))


def smooth_report(models, train_data, val_data, test_data, test_labels, sigma, n0=100, n=100_000, alpha=0.001, over="mfcc",
                  standardize="before", test_filenames=None, domain="22k", limit=None, radii=None, seed=0):
    """Randomized smoothing (lipasr.smoothing.Smooth.certify: Cohen's CERTIFY with N(0, sigma^2 I)) per model: the certified
    accuracy at a grid of L2 radii -- the share of test rows whose smoothed class is the label and whose certified radius is at
    least r -- and the abstention rate.  It certifies the SMOOTHED classifier; next to it, for the constrained model over MFCC rows,
    the median radius its Lipschitz bound certifies for the base classifier (margin / (sqrt(2) get_lipschitz_bound(model))).
    ``over``, ``standardize``, ``test_filenames``, ``domain`` and ``limit`` as in radius_report; ``test_labels`` one-hot, row for
    row with the test rows (over audio: with ``test_filenames``); ``radii``: the grid (default SMOOTH_RADII x sigma).
    Returns {model name: {"radius", "class", "p_lower": the per-row arrays, "radii", "certified_accuracy" (one per radius),
    "abstained", "lipschitz_median" (or None)}}."""
    from .smoothing import Smooth

    if not (float(sigma) >= 0.0 and np.isfinite(float(sigma))):
        raise ValueError(f"sigma = {sigma}: a finite, non-negative number is required")
    rows = _TestRows(models, train_data, val_data, test_data, over, standardize, test_filenames, domain, limit)
    truth = np.asarray(rows.limited(test_labels)).argmax(axis=1)
    radii = np.asarray([f * float(sigma) for f in SMOOTH_RADII] if radii is None else radii, dtype=np.float64)
    kw = dict(n0=n0, n=n, alpha=alpha)
    out = {}
    for name, model in models.items():
        r = {"radius": np.zeros(rows.n), "class": np.full(rows.n, -1, dtype=np.int64), "p_lower": np.zeros(rows.n)}
        for clf, x, lt, idx in rows.batches(model):
            part = Smooth(clf, sigma, seed=seed).certify(x, lengths=lt, **kw)
            for k in r:
                r[k][idx] = part[k]
        lip = None
        if over == "mfcc" and name == "constrained" and rows.n and model._n_classes > 1:
            top = torch.topk(model.predict_device(A._to_dev(rows.x), logits=True).double(), 2, dim=1).values
            lip = float(np.median((top[:, 0] - top[:, 1]).cpu().numpy() / (np.sqrt(2.0) * get_lipschitz_bound(model))))
        hit = r["class"] == truth[:len(r["class"])]
        r["radii"] = radii
        r["certified_accuracy"] = np.array([float(np.mean(hit & (r["radius"] >= q))) if len(hit) else float("nan") for q in radii])
        r["abstained"] = float(np.mean(r["class"] < 0)) if len(hit) else float("nan")
        r["lipschitz_median"] = lip
        out[name] = r
        tag = _tag(name)
        what = f"{len(hit)} test {rows.what}"
        for q, a in zip(radii, r["certified_accuracy"]):
            print(f"Certified accuracy of the smoothed classifier (sigma {sigma}) over {what}{tag} at L2 radius {q}: {a * 100}%")
        print(f"Share of {what} on which the smoothed classifier abstains{tag}: {r['abstained'] * 100}%")
        if lip is not None:
            print(f"Median radius the Lipschitz bound certifies for the base classifier over {what}{tag}: {lip}")
    return out


def _noise_files(noise_dir, n_classes):
    """The files the dataset construction set aside for the audio attacks (:298-304) -> (file names, their one-hot labels)."""
    import os

    return (np.load(os.path.join(noise_dir, "test_filenames.npy")).tolist(),
            to_categorical(np.load(os.path.join(noise_dir, "test_label.npy")), n_classes))


def main(argv=None):
    ap = argparse.ArgumentParser(description="attacks.py's evaluation menu as flags")
    ap.add_argument("--path", default="processed_google_dataset/")
    ap.add_argument("--noise-dir", default="test_dataset_to_add_noise")
    ap.add_argument("--constrained", default="bin/models_constrained/model_constrained_Rho01_dropout01.h5")
    ap.add_argument("--unconstrained", default="bin/models/baseline.h5")
    ap.add_argument("--standardize", choices=["before", "after"], default="before")
    ap.add_argument("--attack", choices=["black", "white", "dolphin", "lipschitz", "radius", "smooth", "certify"], default="black")
    ap.add_argument("--kind", default="simple", help="black: simple|mixture|snr|genetic|square|hsj|warp; white: fgsm|l2|linf|pgd|apgd|auto|universal|jsma|imperceptible|warp")
    ap.add_argument("--pop-size", type=int, default=None, help="black genetic: members per clip (default: GeneticAttack's)")
    ap.add_argument("--max-iter", type=int, default=None, help="black genetic: generations at most (default: GeneticAttack's); black square: queries per clip (default: SquareAttack's); white apgd: iterations (default: 100); white universal: passes over the fitting rows at most (default: UniversalPerturbation's)")
    ap.add_argument("--loss", choices=["ce", "dlr"], default="ce", help="white apgd: cross-entropy or the Difference-of-Logits-Ratio loss")
    ap.add_argument("--over", choices=["audio", "mfcc"], default="mfcc")
    ap.add_argument("--points", type=int, default=None, help="keep only the first N grid points (white imperceptible: the first N files)")
    ap.add_argument("--norm", choices=["inf", "1", "2"], default="inf", help="white fgsm|pgd: ART's norm keyword; white apgd, auto, universal and radius: 2 or inf")
    ap.add_argument("--eps", type=float, default=None, help="white imperceptible: L-inf radius of stage 1, an amplitude (required)")
    ap.add_argument("--learning-rate-1", type=float, default=None, help="white imperceptible: sign-step size of stage 1 (required)")
    ap.add_argument("--learning-rate-2", type=float, default=None, help="white imperceptible: gradient-step size of stage 2 (required)")
    ap.add_argument("--method", choices=["ibp", "crown-ibp"], default="crown-ibp", help="certify: interval bounds alone, or with the backward relaxation pass")
    ap.add_argument("--bounds", action="store_true", help="radius: also the radius bound propagation certifies (MFCC rows)")
    ap.add_argument("--sigma", type=float, default=None, help="smooth: standard deviation of the smoothing noise (required)")
    ap.add_argument("--n0", type=int, default=100, help="smooth: draws that select the class")
    ap.add_argument("--n", type=int, default=100000, help="smooth: draws that estimate its vote share")
    ap.add_argument("--alpha", type=float, default=0.001, help="smooth: failure probability of the certificate")
    ap.add_argument("--room", type=int, default=None, help="white|black over audio: rooms per bank -- the attack is also made through R synthetic rooms and all is heard through R others")
    ap.add_argument("--room-taps", type=int, default=2048, help="--room: samples of each room impulse response")
    ap.add_argument("--room-t60", type=float, nargs=2, default=(0.15, 0.5), metavar=("LO", "HI"), help="--room: range of the reverberation time in seconds")
    ap.add_argument("--room-seed", type=int, default=0, help="--room: seed of the two banks")
    ap.add_argument("--defence", default=None, metavar="SPEC", help="white|black over audio: an input-transformation defence in front of the models, e.g. median:5,lowpass:4000:101,quantize:8 (also bandpass:LO:HI[:TAPS]) -- accuracy undefended, static, adaptive and the detector's hit rate")
    ap.add_argument("--defence-backward", choices=["chain", "identity"], default="chain", help="--defence: the adaptive attack differentiates through the defence, or takes it as the identity on the way back (BPDA)")
    ap.add_argument("--detect-fpr", type=float, default=0.05, help="--defence: false-positive rate the detector's threshold is fitted to on the clean half")
    ap.add_argument("--shift", action="store_true", help="white universal: every clip meets the noise at a random offset")
    ap.add_argument("--length", type=int, default=None, help="white universal: the period of the noise in positions of a row (default: the row width)")
    ap.add_argument("--max-shift-ms", type=float, nargs="+", default=None, help="kind warp: the grid of largest delays in milliseconds (default: 0 2 5 10 20 50 100)")
    ap.add_argument("--max-rate", type=float, default=1.0, help="kind warp: speeds from 1 / R to R (1 to 1.25)")
    ap.add_argument("--max-gain-db", type=float, default=0.0, help="kind warp: levels from -G to +G dB")
    ap.add_argument("--refine", type=int, default=0, help="white warp: first-order steps on each clip's triple after the grid")
    ap.add_argument("--max-iter-1", type=int, default=1000)
    ap.add_argument("--max-iter-2", type=int, default=4000)
    args = ap.parse_args(argv)
    if args.attack == "radius" and args.norm == "1":
        raise ValueError("--attack radius runs DeepFool in --norm 2 or inf")
    if args.attack == "certify" and (args.norm == "1" or args.over != "mfcc"):
        raise ValueError("--attack certify propagates bounds over MFCC rows in --norm inf or 2")
    universal = args.attack == "white" and args.kind == "universal"
    if (args.shift or args.length is not None) and not universal:
        raise ValueError("--shift and --length go with --kind universal")
    if args.attack == "white" and args.kind in ("apgd", "auto", "universal") and args.norm == "1":
        raise ValueError(f"--kind {args.kind} runs in --norm inf or 2")
    if args.attack == "black" and args.kind == "hsj" and args.norm == "1":
        raise ValueError("--kind hsj runs in --norm inf or 2")

    warp = args.attack in ("black", "white") and args.kind == "warp"
    if warp and args.over != "audio":
        raise ValueError("--kind warp resamples audio: give --over audio")
    if warp and args.attack == "black" and args.refine:
        raise ValueError("--refine takes gradients: give --attack white")
    if not warp and (args.max_shift_ms is not None or args.max_rate != 1.0 or args.max_gain_db != 0.0 or args.refine):
        raise ValueError("--max-shift-ms, --max-rate, --max-gain-db and --refine go with --kind warp")

    if args.attack == "smooth" and (args.sigma is None or not 0.0 <= args.sigma < float("inf")):
        raise ValueError("--attack smooth needs --sigma, the standard deviation of the noise (finite, not negative; there is no default)")

    if args.defence is None and (args.defence_backward != "chain" or args.detect_fpr != 0.05):
        raise ValueError("--defence-backward and --detect-fpr go with --defence")
    if args.defence is not None:
        if args.attack not in ("white", "black") or args.over != "audio" or warp or universal:
            raise ValueError("--defence goes with --attack white or black and --over audio (kinds " + ", ".join(OVER_THE_AIR_KINDS) + ")")
        if args.room is not None:
            raise ValueError("--defence and --room are two sweeps: give one of them")
        if args.kind not in OVER_THE_AIR_KINDS:
            raise ValueError(f"--defence takes an attack that optimises within a radius -- {', '.join(OVER_THE_AIR_KINDS)} -- not {args.kind!r}")

    train_data, _, val_data, _, test_data, test_label = A.load_npy_dataset(args.path)
    n_classes = int(test_label.max()) + 1
    labels = to_categorical(test_label, n_classes)
    models = {"constrained": load_model(args.constrained), "unconstrained": load_model(args.unconstrained)}
    names = None
    if args.over == "audio" or args.attack == "dolphin":
        names, labels = _noise_files(args.noise_dir, n_classes)
    if warp:
        return time_warp_sweep(models, train_data, val_data, test_data, labels, names, max_rate=args.max_rate, max_gain_db=args.max_gain_db,
                               refine_steps=args.refine, rooms=args.room, room_taps=args.room_taps, room_t60=tuple(args.room_t60),
                               room_seed=args.room_seed, standardize=args.standardize, grid=args.max_shift_ms, points=args.points)
    if universal:
        if args.room is not None and args.over != "audio":
            raise ValueError("--room goes with --attack white or black and --over audio")
        kw = {k: v for k, v in (("max_iter", args.max_iter), ("length", args.length)) if v is not None}
        return universal_sweep(models, train_data, val_data, test_data, labels, over=args.over, standardize=args.standardize,
                               test_filenames=names, norm=np.inf if args.norm == "inf" else 2, rooms=args.room, room_taps=args.room_taps,
                               room_t60=tuple(args.room_t60), room_seed=args.room_seed, points=args.points, random_shift=args.shift, **kw)
    if args.room is not None or args.defence is not None:
        if args.attack not in ("white", "black") or args.over != "audio":
            raise ValueError("--room goes with --attack white or black and --over audio")
        kw = {k: v for k, v in (("pop_size", args.pop_size if args.kind == "genetic" else None),
                                ("max_iter", args.max_iter if args.kind in ("genetic", "square", "apgd") else None)) if v is not None}
        if args.norm != "inf":
            if args.kind not in ("fgsm", "pgd", "apgd", "auto"):
                raise ValueError("--norm applies to --kind fgsm, pgd, apgd and auto")
            kw["norm"] = int(args.norm)
        if args.kind == "apgd":
            kw["loss_type"] = {"ce": "cross_entropy", "dlr": "difference_logits_ratio"}[args.loss]
        if args.defence is not None:
            return defended_sweep(models, train_data, val_data, test_data, labels, names, args.defence, kind=args.kind,
                                  backward=args.defence_backward, detect_fpr=args.detect_fpr, standardize=args.standardize,
                                  points=args.points, **kw)
        return over_the_air_sweep(models, train_data, val_data, test_data, labels, names, kind=args.kind, rooms=args.room,
                                  room_taps=args.room_taps, room_t60=tuple(args.room_t60), room_seed=args.room_seed,
                                  standardize=args.standardize, points=args.points, **kw)
    if args.attack == "black":
        if args.kind == "genetic":
            kw = {k: v for k, v in (("pop_size", args.pop_size), ("max_iter", args.max_iter)) if v is not None}
            return genetic_sweep(models, train_data, val_data, test_data, labels, over=args.over, standardize=args.standardize,
                                 test_filenames=names, points=args.points, **kw)
        if args.kind == "square":
            kw = {} if args.max_iter is None else dict(max_iter=args.max_iter)
            return square_sweep(models, train_data, val_data, test_data, labels, over=args.over, standardize=args.standardize,
                                test_filenames=names, points=args.points, **kw)
        if args.kind == "hsj":
            kw = {} if args.max_iter is None else dict(max_iter=args.max_iter)
            return hopskipjump_sweep(models, train_data, val_data, test_data, labels, over=args.over, standardize=args.standardize,
                                     test_filenames=names, norm=np.inf if args.norm == "inf" else 2, points=args.points, **kw)
        return black_box_sweep(models, train_data, val_data, test_data, labels, kind=args.kind, over=args.over,
                               standardize=args.standardize, test_filenames=names, points=args.points)
    if args.attack == "lipschitz":
        return lipschitz_report(models, train_data, val_data, test_data, over=args.over, standardize=args.standardize,
                                test_filenames=names)
    if args.attack == "radius":
        return radius_report(models, train_data, val_data, test_data, over=args.over, standardize=args.standardize,
                             test_filenames=names, norm=np.inf if args.norm == "inf" else 2, limit=args.points,
                             **({"bounds": {}} if args.bounds else {}))
    if args.attack == "certify":
        return certify_report(models, train_data, val_data, test_data, labels, norm=np.inf if args.norm == "inf" else 2,
                              method=args.method, standardize=args.standardize, points=args.points)
    if args.attack == "smooth":
        return smooth_report(models, train_data, val_data, test_data, labels, args.sigma, n0=args.n0, n=args.n, alpha=args.alpha,
                             over=args.over, standardize=args.standardize, test_filenames=names, limit=args.points)
    if args.attack == "dolphin":
        return dolphin_sweep(models, train_data, val_data, test_data, labels, names, standardize=args.standardize, points=args.points)
    if args.kind == "imperceptible":
        if args.over != "audio":
            raise ValueError("--kind imperceptible perturbs audio: give --over audio")
        if args.eps is None or args.learning_rate_1 is None or args.learning_rate_2 is None:
            raise ValueError("--kind imperceptible needs --eps, --learning-rate-1 and --learning-rate-2 (amplitudes; there are no defaults)")
        return imperceptible_report(models, train_data, val_data, test_data, labels, names, args.eps, args.learning_rate_1,
                                    args.learning_rate_2, standardize=args.standardize, limit=args.points, max_iter_1=args.max_iter_1,
                                    max_iter_2=args.max_iter_2)
    kw = {}
    if args.over == "audio":
        kw.update(over="audio", test_filenames=names)
    if args.norm != "inf":
        if args.kind not in ("fgsm", "pgd", "apgd", "auto"):
            raise ValueError("--norm applies to --kind fgsm, pgd, apgd and auto")
        kw["norm"] = int(args.norm)
    if args.kind == "apgd":
        kw["loss_type"] = {"ce": "cross_entropy", "dlr": "difference_logits_ratio"}[args.loss]
        if args.max_iter is not None:
            kw["max_iter"] = args.max_iter
    return white_box_sweep(models, train_data, val_data, test_data, labels, kind=args.kind, standardize=args.standardize,
                           points=args.points, **kw)


if __name__ == "__main__":
    main()
