"""The reference's constrained-training driver (train_constraints.py:63-111) on lipasr.

``get_model()`` and ``lip_stats_callback`` keep the reference's shape; ``main()`` reads like
train_constraints.py:91-111 but trains on synthetic clips (the reference's ``.npy`` features are LFS
pointers that are absent from the mount) pushed through the on-GPU MFCC kernel.
"""
from __future__ import annotations

import argparse

import numpy as np

from .Constraints import customConstraint, norm_constraint, norm_constraint_FISTA, simple_norm_constraint  # noqa: F401
from .attacks import TensorFlowV2Classifier, standardize_dataset
from .extract_features_construct_dataset import get_lipschitz_constrained, get_local_lipschitz, get_norms, mfcc
from .keras import (BatchNormalization, Callback, CategoricalCrossentropy, Dataset, Dense, Dropout, EarlyStopping, Input, Model,
                    ModelCheckpoint, NonNeg, TensorBoard, load_model, to_categorical)
from .synth import synth_clips_fast


def tensorboard_callback():
    """train_constraints.py:45-48."""
    import datetime

    logdir = "logs/log_constrained" + datetime.datetime.now().strftime("%Y%m%d-%H%M%S")
    return TensorBoard(log_dir=logdir)


class lip_stats_callback(Callback):
    """train_constraints.py:52-60: per-layer spectral norms and the network Lipschitz constant each epoch.
    probe= (ours; default None: the reference's output, unchanged): a small array of standardised rows [k, n_in]; the largest
    local Lipschitz constant of the logits over those rows (get_local_lipschitz) is logged as well."""

    def __init__(self, probe=None):
        super().__init__()
        self.probe = None if probe is None else np.asarray(probe, dtype=np.float32)

    def on_epoch_begin(self, epoch, logs=None):
        lip_cst = get_lipschitz_constrained(self.model)
        norms = get_norms(self.model)
        dense = [l for l in self.model.layers if "dense" in l.name]
        for layer, norm in zip(dense, norms):
            print(f"The norm for layer {layer} is : {norm}")
        print(f"The Lipschitz constant on epoch {epoch} is {lip_cst}")
        if self.probe is not None:
            clf = TensorFlowV2Classifier(model=self.model, nb_classes=self.model._n_classes, input_shape=(self.probe.shape[1],))
            local = get_local_lipschitz(clf, self.probe)
            print(f"The largest local Lipschitz constant over {len(local)} probe rows on epoch {epoch} is {local.max()}")


def get_model(n_in=880, n_classes=10, **kw):
    """train_constraints.py:63-88."""
    inp = Input((n_in,))
    hdn = Dense(1024, activation="relu", kernel_constraint=NonNeg())(inp)
    hdn = BatchNormalization()(hdn)
    hdn = Dropout(0.1)(hdn)

    hdn = Dense(512, activation="relu", kernel_constraint=NonNeg())(hdn)
    hdn = BatchNormalization()(hdn)
    hdn = Dropout(0.1)(hdn)

    hdn = Dense(256, activation="relu", kernel_constraint=NonNeg())(hdn)
    hdn = BatchNormalization()(hdn)
    hdn = Dropout(0.1)(hdn)

    hdn = Dense(128, activation="relu", kernel_constraint=NonNeg())(hdn)
    hdn = BatchNormalization()(hdn)

    hdn = Dense(64, activation="relu", kernel_constraint=NonNeg())(hdn)
    hdn = BatchNormalization()(hdn)

    out = Dense(n_classes, activation="softmax", kernel_constraint=NonNeg())(hdn)
    return Model(inputs=inp, outputs=out, **kw)


def get_model_unconstrained(n_in=880, n_classes=10, **kw):
    """train_google_dataset.py:49-74: no NonNeg, Dropout(0.4) after every hidden block."""
    inp = Input((n_in,))
    hdn = inp
    for units in (1024, 512, 256, 128, 64):
        hdn = Dense(units, activation="relu")(hdn)
        hdn = BatchNormalization()(hdn)
        hdn = Dropout(0.4)(hdn)
    out = Dense(n_classes, activation="softmax")(hdn)
    return Model(inputs=inp, outputs=out, **kw)


def synthetic_dataset(n_train=16566, n_dev=4733, n_test=2366, seed=1234):
    """Synthetic stand-in with the reference's split sizes, extracted by the K1 kernel."""
    waves, labels = synth_clips_fast(n_train + n_dev + n_test, seed)
    feats = np.concatenate([mfcc(waves[s:s + 512]).cpu().numpy() for s in range(0, len(waves), 512)]).astype(np.float64)
    a, b = n_train, n_train + n_dev
    return (feats[:a], labels[:a]), (feats[a:b], labels[a:b]), (feats[b:], labels[b:])


def load_processed_dataset(path="processed_google_dataset/"):
    """train_constraints.py:16-25: the six ``.npy`` files extract_features_construct_dataset.main() writes."""
    import os

    def ld(name):
        return np.load(os.path.join(path, name + ".npy"))

    return (ld("train_data"), ld("train_label")), (ld("dev_data"), ld("dev_label")), (ld("test_data"), ld("test_label"))


def add_certified_arguments(ap):
    """The flags of IBP certified training (lipasr.bounds.IBPCrossentropy); without --certified-eps training is unchanged."""
    ap.add_argument("--certified-eps", type=float, default=None, help="train on the interval bounds at this norm-inf radius "
                                                                        "(of the standardised features); default: off")
    ap.add_argument("--certified-kappa", type=float, default=0.5, help="final weight of the robust cross-entropy")
    ap.add_argument("--certified-warmup", type=int, default=0, help="steps of plain training before the ramp")
    ap.add_argument("--certified-ramp", type=int, default=1, help="steps over which eps and kappa rise from 0")
    ap.add_argument("--certified-method", choices=("ibp", "crown-ibp"), default="ibp", help="the margins the robust cross-entropy is "
                    "taken on: the interval bounds (IBPCrossentropy) or their mix with the CROWN-IBP margins (CrownIBPCrossentropy)")
    ap.add_argument("--certified-beta", type=float, nargs=2, default=(1.0, 0.0), metavar=("START", "END"),
                    help="crown-ibp: the weight of the CROWN-IBP margin at the start and at the end of the ramp")
    return ap


def certified_arguments(argv):
    return add_certified_arguments(argparse.ArgumentParser(add_help=False)).parse_known_args(argv)[0]


def certified_loss(args):
    """The IBPCrossentropy or CrownIBPCrossentropy the flags ask for, or None."""
    if args.certified_eps is None:
        return None
    from .bounds import IBPCrossentropy

    if args.certified_method == "crown-ibp":
        from .bounds import CrownIBPCrossentropy

        return CrownIBPCrossentropy(args.certified_eps, kappa=args.certified_kappa, warmup_steps=args.certified_warmup,
                                    ramp_steps=args.certified_ramp, beta_start=args.certified_beta[0], beta_end=args.certified_beta[1])
    return IBPCrossentropy(args.certified_eps, kappa=args.certified_kappa, warmup_steps=args.certified_warmup,
                           ramp_steps=args.certified_ramp)


def add_smooth_arguments(ap):
    """The flags of training for randomized smoothing (lipasr.smoothing.GaussianCrossentropy / MACERCrossentropy); without
    --smooth-sigma training is unchanged.  Mutually exclusive with --certified-eps (smooth_loss refuses both through ap.error)."""
    ap.add_argument("--smooth-sigma", type=float, default=None, help="train on copies with N(0, sigma^2) noise on the standardised "
                                                                       "features, for lipasr.smoothing.Smooth at this sigma; default: off")
    ap.add_argument("--smooth-method", choices=("gaussian", "macer"), default="gaussian", help="cross-entropy on the noisy copies "
                    "(GaussianCrossentropy) or MACER's certified-radius loss (MACERCrossentropy)")
    ap.add_argument("--smooth-draws", type=int, default=None, help="noisy copies per clip and step (default: gaussian 1, macer 16); the "
                                                                     "model is planned for batch x draws rows")
    ap.add_argument("--smooth-lambda", type=float, default=12.0, help="macer: weight of the robust term")
    ap.add_argument("--smooth-gamma", type=float, default=8.0, help="macer: the hinge on Phi^-1(q_y) - Phi^-1(q_B)")
    ap.add_argument("--smooth-beta", type=float, default=16.0, help="macer: inverse temperature of the soft votes")
    ap.add_argument("--smooth-warmup", type=int, default=0, help="macer: steps at lambda 0 before the robust term counts")
    return ap


def smooth_draws(args):
    """Noisy copies per clip the flags ask for (1 without --smooth-sigma): the drivers plan the model for batch x this many rows."""
    if args.smooth_sigma is None:
        return 1
    return args.smooth_draws if args.smooth_draws is not None else (16 if args.smooth_method == "macer" else 1)


def smooth_loss(args, ap=None):
    """The GaussianCrossentropy or MACERCrossentropy the flags ask for, or None.  Together with --certified-eps: an argparse error
    (``ap.error``; a ValueError without a parser)."""
    if args.smooth_sigma is None:
        return None
    if getattr(args, "certified_eps", None) is not None:
        msg = "argument --smooth-sigma: not allowed with argument --certified-eps"
        if ap is not None:
            ap.error(msg)
        raise ValueError(msg)
    from .smoothing import GaussianCrossentropy, MACERCrossentropy

    if args.smooth_method == "macer":
        return MACERCrossentropy(args.smooth_sigma, draws=smooth_draws(args), lam=args.smooth_lambda, gamma=args.smooth_gamma,
                                 beta=args.smooth_beta, warmup_steps=args.smooth_warmup)
    return GaussianCrossentropy(args.smooth_sigma, draws=smooth_draws(args))


def main(argv=None):
    ap = add_smooth_arguments(add_certified_arguments(argparse.ArgumentParser()))
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--rho", type=float, default=0.1)
    ap.add_argument("--small", action="store_true", help="2048/512/512 clips instead of the reference's split sizes")
    ap.add_argument("--data", default=None, help="directory with train/dev/test _data.npy and _label.npy "
                                                 "(train_constraints.py:16-25); default: synthetic clips")
    args = ap.parse_args(argv)
    sizes = (2048, 512, 512) if args.small else (16566, 4733, 2366)
    if args.data:
        (train_data, train_label), (val_data, val_label), (test_data, test_label1) = load_processed_dataset(args.data)
    else:
        (train_data, train_label), (val_data, val_label), (test_data, test_label1) = synthetic_dataset(*sizes)
    train_label, val_label, test_label = (to_categorical(l, 10) for l in (train_label, val_label, test_label1))
    train_data, val_data, test_data = standardize_dataset(train_data, val_data, test_data)

    train_dataset = Dataset.from_tensor_slices((train_data, train_label)).shuffle(880, reshuffle_each_iteration=False).batch(512)
    val_dataset = Dataset.from_tensor_slices((val_data, val_label)).shuffle(880, reshuffle_each_iteration=False).batch(512)

    loss = smooth_loss(args, ap) or certified_loss(args) or CategoricalCrossentropy()
    model = get_model(**({"max_batch": max(1024, 512 * smooth_draws(args))} if args.smooth_sigma is not None else {}))
    model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
    print(model.summary())
    model.fit(train_dataset, epochs=args.epochs, validation_data=val_dataset, verbose=2,
              callbacks=[EarlyStopping(monitor="val_loss", patience=6000, restore_best_weights=False),
                         simple_norm_constraint(rho=args.rho, affected_layers_indices=[]),
                         lip_stats_callback(),
                         ModelCheckpoint("bin/models_constrained/TEST.h5", save_best_only=True, verbose=1)])
    model = load_model("bin/models_constrained/TEST.h5")
    y = np.argmax(model.predict(test_data), axis=1)
    results = model.evaluate(test_data, test_label)
    print(f"Test loss: {results[0]} / Test accuracy: {results[1]} / agreement {np.mean(y == test_label1)}")


if __name__ == "__main__":
    main()
