"""HIP-event timing of the legs of one HopSkipJump iteration, in both norms: 1024 perturbed rows x 880 features (16 clips x 64 draws,
TensorFlowV2Classifier) and 32 rows x 22 050 samples (4 clips x 8 draws, WaveformClassifier, domain "22k"): lipasr_hsj_expand, the
estimator's forward pass over those rows, lipasr_hsj_accumulate and lipasr_hsj_direction; then one query of the bisection:
the estimator over the clips' candidates and lipasr_hsj_search.  The question the numbers answer: what share of an iteration is
ours and what share is the estimator's.  One process, whole chip, medians over --iters calls after --warm warm-up calls, repeated
--repeats times for the spread (profiles/hsj_timing.txt)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, keras as K, train_constraints as T
from lipasr.attacks import TensorFlowV2Classifier, WaveformClassifier
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.hopskipjump import BISECT, FIRST, START, hsj_accumulate, hsj_direction, hsj_expand, hsj_search

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
print(f"library {os.path.relpath(N.LIB_PATH, ROOT)} version {N.lib.lipasr_version()}", flush=True)


def timed(name, fn):
    meds = []
    for _ in range(args.repeats):
        for _ in range(args.warm): fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
        ev[0].record()
        for i in range(args.iters):
            fn(); ev[i + 1].record()
        torch.cuda.synchronize()
        t = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]) * 1e3
        meds.append(float(np.median(t)))
    print(f"  {name:58s} median {np.median(meds):8.1f} us  (medians of {args.repeats} runs: {min(meds):.1f} .. {max(meds):.1f}; last run min {t.min():.1f} p90 "
          f"{np.percentile(t, 90):.1f})", flush=True)
    return float(np.median(meds))


def run(name, clf, x, draws):
    B, n = x.shape
    clip = clf.clip_values
    print(f"{name}: {B} clips x {draws} draws = {B * draws} rows x {n}", flush=True)
    labels = clf.predict_device(x, logits=True).argmax(dim=1).to(torch.int32)
    delta = torch.full((B,), 0.05, device=dev)
    rows = torch.empty(B * draws, n, device=dev)
    sums, counts = torch.zeros(B, 2, n, dtype=torch.float64, device=dev), torch.zeros(B, 2, dtype=torch.int32, device=dev)
    b = {k: torch.empty(B, n, device=dev) for k in ("x_cand", "x_far", "x_adv", "x_best", "u")}
    fstate, istate = torch.zeros(B, 8, device=dev), torch.ones(B, 8, dtype=torch.int32, device=dev)
    one = torch.ones(B, device=dev)
    for norm in (2, np.inf):
        tag = f"norm {norm}"
        t_e = timed(f"lipasr_hsj_expand ({tag})", lambda: hsj_expand(x, delta, draws, 1, 1, norm, out=rows, clip_values=clip))
        z = clf.predict_device(rows, logits=True)
        t_p = timed(f"estimator leg: predict_device over the {B * draws} rows", lambda: clf.predict_device(rows, logits=True))
        t_a = timed("lipasr_hsj_accumulate", lambda: hsj_accumulate(z, labels, rows, x, sums=sums, counts=counts))
        t_d = timed(f"lipasr_hsj_direction ({tag})", lambda: hsj_direction(sums, counts, norm, u=b["u"]))
        ours = t_e + t_a + t_d
        print(f"  one estimate, {tag}: ours {ours:.1f} us + estimator {t_p:.1f} us = {ours + t_p:.1f} us; ours is {100 * ours / (ours + t_p):.1f} % of it", flush=True)
        kw = dict(labels=labels, x0=x, seed=1, norm=norm, fstate=fstate, istate=istate, start_lo=-one, start_hi=one, theta=one * 0.0, clip_values=clip,
                  classes=clf.nb_classes, **b)
        hsj_search(None, mode=START, flags=FIRST, **kw)
        b["x_far"].copy_(rows[::draws])
        zc = clf.predict_device(b["x_cand"], logits=True).clone()

        def reopen():  # every row bisects again from the same far point: theta 0, so the interval never closes on its own
            istate[:, N.HSJ_I["ok"]] = 1
            hsj_search(None, mode=BISECT, flags=FIRST, **kw)
        reopen()
        t_q = timed(f"estimator leg: predict_device over the {B} candidates", lambda: clf.predict_device(b["x_cand"], logits=True))
        t_s = timed(f"lipasr_hsj_search (BISECT, {tag})", lambda: (reopen() if not bool(istate[:, 0].all()) else None, hsj_search(zc, mode=BISECT, flags=0, **kw)))
        print(f"  one query, {tag}: search {t_s:.1f} us + estimator {t_q:.1f} us = {t_s + t_q:.1f} us; the search is {100 * t_s / (t_s + t_q):.1f} % of it "
              f"(the search figure includes one look at the active flags from the host)", flush=True)


rng = np.random.default_rng(7)
K.reset_layer_names()
m = T.get_model_unconstrained(max_batch=1024)
m.compile(optimizer="adam", loss=K.CategoricalCrossentropy(), metrics=["accuracy"])
clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
run("features", clf, torch.as_tensor(rng.standard_normal((16, 880)).astype(np.float32)).to(dev), 64)
ex = MfccExtractor(16000, 16000, batch_max=32)
wclf = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
run("audio", wclf, torch.as_tensor((0.1 * rng.standard_normal((4, 22050))).astype(np.float32)).to(dev), 8)
ex.close()
