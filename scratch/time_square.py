"""HIP-event timing of one Square Attack query at B = 1024 rows x 880 features (TensorFlowV2Classifier, rows as 20 x 44 pictures) and
x 22 050 samples (WaveformClassifier, domain "22k", strips): lipasr_square_step beside the estimator's forward pass it follows, at
the first window of the schedule (p = 0.4 of the row) and at a late one (p = 0.8 / 512), and lipasr_square_init; then the queries
per second of SquareAttack against GeneticAttack(pop_size=20) on the same rows, host clock around whole generate_device calls that
end in a synchronise (both attacks at an eps no row leaves its class at, so that neither stops early).  One process, whole chip,
medians over --iters calls after --warm warm-up calls, repeated --repeats times for the spread (profiles/square_timing.txt)."""
import sys, os, argparse, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, keras as K, train_constraints as T
from lipasr.attacks import GeneticAttack, SquareAttack, TensorFlowV2Classifier, WaveformClassifier
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.square import square_init, square_p_q, square_step, square_window

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--rows", type=int, default=1024); ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--queries", type=int, default=200, help="SquareAttack max_iter of the queries-per-second runs")
args = ap.parse_args()
dev = torch.device("cuda", 0)
B = args.rows
print(f"library {os.path.relpath(N.LIB_PATH, ROOT)} version {N.lib.lipasr_version()}: {B} rows", flush=True)


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
    print(f"  {name:62s} median {np.median(meds):8.1f} us  (medians of {args.repeats} runs: {min(meds):.1f} .. {max(meds):.1f}; last run min {t.min():.1f} p90 "
          f"{np.percentile(t, 90):.1f})", flush=True)
    return float(np.median(meds))


def run(name, clf, x0, shape, eps):
    n = x0.shape[1]
    height, width = shape
    print(f"{name}: {B} x {n} as {height} x {width}", flush=True)
    clip = clf.clip_values
    best, cand = torch.empty_like(x0), torch.empty_like(x0)
    win, loss = torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, device=dev)
    done = torch.zeros(B, dtype=torch.int32, device=dev)
    kw = dict(x_best=best, x_cand=cand, win=win, clip_values=clip)
    square_init(x0, height, width, 0, 1, eps, **kw)
    z = clf.predict_device(cand, logits=True)
    labels = z.argmax(dim=1).to(torch.int32)
    z = z.clone()
    z[torch.arange(B, device=dev), labels.long()] += 100.0  # a margin no proposal beats: every row stays in the search
    t_i = timed("lipasr_square_init", lambda: square_init(x0, height, width, 0, 1, eps, **kw))
    t_p = timed("estimator leg: predict_device(x_cand, logits=True)", lambda: clf.predict_device(cand, logits=True))
    out = {}
    for tag, p in (("first window, p = 0.4", 0.4), ("late window, p = 0.8 / 512", 0.8 / 512)):
        wh, ww = square_window(p, height, width)
        it = [1]

        def step():
            square_step(z, labels, x0, height, width, wh, ww, square_p_q(p), 0, it[0], 1, eps, loss_best=loss, done=done, **kw)
            it[0] += 1
        square_step(z, labels, x0, height, width, wh, ww, square_p_q(p), 0, 0, 1, eps, loss_best=loss, done=done, **kw)
        out[tag] = timed(f"lipasr_square_step ({tag}: {wh} x {ww} = {wh * ww} elements)", step)
        torch.cuda.synchronize()
        assert int((done != 0).sum()) == 0 and int((win[:, 2] * win[:, 3] == wh * ww).sum()) == B
    for tag, t in out.items():
        print(f"  one query, {tag}: step {t:.1f} us + estimator {t_p:.1f} us = {t + t_p:.1f} us; the step is {100 * t / (t + t_p):.1f} % of it", flush=True)
    return t_p


def qps(name, clf, x0, shape, eps):
    """Queries per second of whole attacks: rows x queries per row over the wall time of generate_device (ends in a synchronise)."""
    rows = x0.shape[0]
    sq = SquareAttack(clf, eps=eps, max_iter=args.queries, batch_size=rows, shape=shape, seed=1)
    gens = max(1, args.queries // 20)
    ga = GeneticAttack(clf, eps, pop_size=20, max_iter=gens, seed=1)
    res = {}
    for tag, atk, per_row in (("SquareAttack", sq, args.queries), ("GeneticAttack(pop_size=20)", ga, 20 * gens)):
        atk.generate_device(x0); torch.cuda.synchronize()  # warm-up
        rates = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            atk.generate_device(x0); torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            spent = int(atk.queries_.sum())
            rates.append(spent / dt)
        if bool(atk.success_.any()) or spent != rows * per_row:
            print(f"  ({int(atk.success_.sum())} rows left their class and stopped early: {spent} queries spent, not {rows * per_row})")
        res[tag] = float(np.median(rates))
        print(f"  {name}: {tag:28s} {per_row} queries per row x {rows} rows: median {np.median(rates) / 1e6:7.3f} M queries/s "
              f"({min(rates) / 1e6:.3f} .. {max(rates) / 1e6:.3f} over {args.repeats} runs)", flush=True)
    print(f"  {name}: SquareAttack answers {res['SquareAttack'] / res['GeneticAttack(pop_size=20)']:.2f} x the queries per second of GeneticAttack", flush=True)


rng = np.random.default_rng(7)
K.reset_layer_names()
m = T.get_model_unconstrained(max_batch=max(B, 20 * 64))
m.compile(optimizer="adam", loss=K.CategoricalCrossentropy(), metrics=["accuracy"])
clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
xf = torch.as_tensor(rng.standard_normal((B, 880)).astype(np.float32)).to(dev)
run("features", clf, xf, (20, 44), 0.1)
ex = MfccExtractor(16000, 16000, batch_max=max(B, 20 * 64))
wclf = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
x22 = torch.as_tensor((0.1 * rng.standard_normal((B, 22050))).astype(np.float32)).to(dev)
run("audio", wclf, x22, (1, 22050), 0.002)
print("queries per second (whole attacks, host clock):", flush=True)
qps("features", clf, xf, (20, 44), 1e-6)
qps("audio", wclf, x22[:64].contiguous(), None, 1e-9)
ex.close()
