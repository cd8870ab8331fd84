"""HIP-event timing of one generation of the genetic black-box attack at 1024 population rows (B = 64 clips, P = 16 members) x
22 050 samples (WaveformClassifier, domain "22k") and x 880 features (TensorFlowV2Classifier): lipasr_genetic_breed,
lipasr_genetic_select, the classifier leg between them, and the same generation composed from torch ops (torch.rand, gather,
where, clamp) with its launch count -- the yardstick, there being no parent-commit number.  One process, whole chip, medians over
--iters calls after --warm warm-up calls (profiles/genetic_timing.txt)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, keras as K, train_constraints as T
from lipasr.attacks import TensorFlowV2Classifier, WaveformClassifier
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.genetic import genetic_breed, genetic_select, mutate_threshold

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--clips", type=int, default=64); ap.add_argument("--pop", type=int, default=16)
ap.add_argument("--mutation-p", type=float, default=0.0005)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, P = args.clips, args.pop
rows = B * P
print(f"library {os.path.relpath(N.LIB_PATH, ROOT)} version {N.lib.lipasr_version()}: {B} clips x {P} members = {rows} rows, mutation_p {args.mutation_p}", flush=True)


def timed(name, fn, nbytes=None):
    for _ in range(args.warm): fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
    ev[0].record()
    for i in range(args.iters):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    t = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]) * 1e3
    med = float(np.median(t))
    rate = "" if nbytes is None else f"   {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.2f} TB/s  ({nbytes / 8e12 * 1e6:6.1f} us at 8 TB/s)"
    print(f"  {name:58s} median {med:9.1f} us  min {t.min():9.1f}  p90 {np.percentile(t, 90):9.1f}{rate}", flush=True)
    return med


def launches(fn):
    """Kernel launches of one call, counted by the profiler of torch (a separate, untimed call)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(); torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and e.device_time_total > 0)


def torch_generation(x0, pop, parents, step, eps, lo, hi, p_mut):
    """The generation of lipasr_genetic_breed from torch ops: two gathers, three random tensors, where, clamp (its own random
    stream: the same work, not the same bits).  The elite and the padding are left out: less work than the kernel does."""
    b, n = x0.shape
    pv = pop.view(b, P, n)
    ia = parents[:, :, 0].long().clamp_(0, P - 1)[:, :, None].expand(b, P, n)
    ic = parents[:, :, 1].long().clamp_(0, P - 1)[:, :, None].expand(b, P, n)
    a, c = torch.gather(pv, 1, ia), torch.gather(pv, 1, ic)
    child = torch.where(torch.rand(b, P, n, device=x0.device) < 0.5, a, c)
    mut = torch.rand(b, P, n, device=x0.device) < p_mut
    child = torch.where(mut, child + step * (2.0 * torch.rand(b, P, n, device=x0.device) - 1.0), child)
    x = x0[:, None, :]
    child = torch.maximum(torch.minimum(child, x + eps), x - eps).clamp_(lo, hi)
    return child.view(b * P, n)


def torch_select(z, labels, T_):
    """lipasr_genetic_select from torch ops (untargeted): margin, argmax, softmax weights, two multinomial draws per child."""
    b = labels.shape[0]
    zy = z.gather(1, labels.long().repeat_interleave(P)[:, None])
    other = z.scatter(1, labels.long().repeat_interleave(P)[:, None], -float("inf")).max(dim=1).values
    fit = (other - zy[:, 0]).view(b, P)
    best = fit.argmax(dim=1)
    w = torch.softmax(fit / T_, dim=1)
    par = torch.multinomial(w, 2 * P, replacement=True).view(b, P, 2).to(torch.int32)
    par[:, 0, 0] = best.to(torch.int32); par[:, 0, 1] = -1
    return fit, best, (fit.gather(1, best[:, None]) > 0)[:, 0], par


def run(name, clf, x0, lrep, eps):
    n = x0.shape[1]
    print(f"{name}: {rows} x {n}", flush=True)
    thresh, seed = mutate_threshold(args.mutation_p), 1
    clip = clf.clip_values if isinstance(clf, WaveformClassifier) else None
    lo, hi = (-float("inf"), float("inf")) if clip is None else clip
    bufs = [torch.empty(rows, n, device=dev) for _ in range(2)]
    fitness = torch.empty(B, P, device=dev); best = torch.zeros(B, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.int32, device=dev); parents = torch.empty(B, P, 2, dtype=torch.int32, device=dev)
    labels = torch.zeros(B, dtype=torch.int32, device=dev)
    predict = (lambda r: clf.predict_device(r, logits=True, lengths=lrep)) if isinstance(clf, WaveformClassifier) else \
        (lambda r: clf.model.predict_device(r, logits=True))
    genetic_breed(x0, P, 0, seed, thresh, eps, eps, clip_values=clip, out=bufs[0])
    z = predict(bufs[0])
    labels.copy_(z.view(B, P, -1)[:, 0].argmax(dim=1))
    # a label that no member leaves at this eps keeps every clip running: fitness <= 0, parents drawn
    genetic_select(z, labels, P, 0, seed, 0.01, fitness=fitness, best=best, done=done, parents=parents)
    torch.cuda.synchronize()
    print(f"  clips done after the first generation (their children are copies): {int((done != 0).sum())} of {B}")
    moved = 16 * rows * n
    t_b = timed("lipasr_genetic_breed (two parents)", lambda: genetic_breed(x0, P, 1, seed, thresh, eps, eps, pop_in=bufs[0], parents=parents,
                                                                         clip_values=clip, out=bufs[1]), moved)
    timed("lipasr_genetic_breed (initial population, pop_in NULL)", lambda: genetic_breed(x0, P, 0, seed, thresh, eps, eps, clip_values=clip, out=bufs[1]))
    t_p = timed("classifier leg: predict_device(pop, logits=True)", lambda: predict(bufs[0]))

    def sel():
        done.zero_()
        genetic_select(z, labels, P, 0, seed, 0.01, fitness=fitness, best=best, done=done, parents=parents)
    t_z = timed("done.zero_() alone", lambda: done.zero_())
    t_s = timed("lipasr_genetic_select + done.zero_()", sel)
    t_tb = timed("torch ops: breed (rand x3, gather x2, where, clamp)", lambda: torch_generation(x0, bufs[0], parents, eps, eps, lo, hi, args.mutation_p), moved)
    t_ts = timed("torch ops: select (margin, softmax, multinomial)", lambda: torch_select(z, labels, 0.01))
    print(f"  kernel pair {t_b + t_s - t_z:.1f} us against torch ops {t_tb + t_ts:.1f} us: {(t_tb + t_ts) / (t_b + t_s - t_z):.2f} x; "
          f"one generation with the classifier: {t_b + t_s - t_z + t_p:.1f} us, of which the classifier {t_p:.1f}", flush=True)
    return name, dict(breed=lambda: genetic_breed(x0, P, 1, seed, thresh, eps, eps, pop_in=bufs[0], parents=parents, clip_values=clip, out=bufs[1]),
                      select=lambda: genetic_select(z, labels, P, 0, seed, 0.01, fitness=fitness, best=best, done=done, parents=parents),
                      torch_breed=lambda: torch_generation(x0, bufs[0], parents, eps, eps, lo, hi, args.mutation_p),
                      torch_select=lambda: torch_select(z, labels, 0.01))


rng = np.random.default_rng(7)
K.reset_layer_names()
m = T.get_model_unconstrained(max_batch=rows)
m.compile(optimizer="adam", loss=K.CategoricalCrossentropy(), metrics=["accuracy"])
clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
counted = [run("features", clf, torch.as_tensor(rng.standard_normal((B, 880)).astype(np.float32)).to(dev), None, 0.1)]
ex = MfccExtractor(16000, 16000, batch_max=rows)
wclf = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
x22 = torch.as_tensor((0.1 * rng.standard_normal((B, 22050))).astype(np.float32)).to(dev)
counted.append(run("audio", wclf, x22, None, 0.002))
# last, so that a profiler that does not work here costs no timing
for name, fns in counted:
    try:
        print(f"{name}: launches per call: " + ", ".join(f"{k} {launches(fn)}" for k, fn in fns.items()), flush=True)
    except Exception as e:  # the timings above stand
        print(f"{name}: launches not counted ({type(e).__name__}: {e})", flush=True)
ex.close()
