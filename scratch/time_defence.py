"""HIP-event timing of the input-transformation defences at the shape an adaptive attack runs them: 1 024 rows of 22 050 samples
under the three-stage chain median 5 -> low-pass 4 kHz (101 taps) -> 8 bits -- lipasr_defence_apply and lipasr_defence_vjp as ONE
launch each, the same chain as three single-stage launches per direction (the intermediates through memory: the comparison that
justifies the fusion), each stage alone, and, on the same run, one WaveformClassifier.loss_gradient_device pass over the same rows
(domain "22k"), which is what the defence sits in front of.  One process, whole chip, medians over --iters calls after --warm
warm-up calls, repeated --repeats times for the spread (profiles/defence_timing.txt)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, train_constraints as T
from lipasr.attacks import DefendedClassifier, WaveformClassifier
from lipasr.defences import AudioDefence, lowpass_taps
from lipasr.extract_features_construct_dataset import MfccExtractor

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=30); ap.add_argument("--warm", type=int, default=5)
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
        t = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)])
        meds.append(float(np.median(t)))
    med = float(np.median(meds))
    print(f"  {name:72s} median {med:8.3f} ms  (medians of {args.repeats} runs: {min(meds):.3f} .. {max(meds):.3f}; last run min {t.min():.3f} "
          f"p90 {np.percentile(t, 90):.3f})", flush=True)
    return med


rows, n = 1024, 22050
rng = np.random.default_rng(0)
x = torch.as_tensor(rng.uniform(-0.5, 0.5, (rows, n)).astype(np.float32)).to(dev)
g = torch.as_tensor(rng.uniform(-1, 1, (rows, n)).astype(np.float32)).to(dev)
stages = [("median", 5), ("lowpass", lowpass_taps(4000, 22050, 101)), ("quantize", 8)]
fused = AudioDefence(stages)
singles = [AudioDefence([st]) for st in stages]
bufs = [torch.empty(rows, n, device=dev) for _ in range(4)]
gb = [torch.empty(rows, n, device=dev) for _ in range(2)]
gf = torch.empty(rows, n, device=dev)


def composed_apply():
    u = x
    for d, o in zip(singles, bufs[:3]):
        u = d.apply(u, out=o)
    return u


def composed_vjp():
    """The forward pass has left every stage's input in bufs; the three adjoints in reverse."""
    d3, d2, d1 = singles[::-1]
    d3.vjp(bufs[1], g, out=gb[0])
    d2.vjp(bufs[0], gb[0], out=gb[1])
    return d1.vjp(x, gb[1], out=gb[0])


print(f"{rows} rows x {n}, chain median 5 -> low-pass 101 taps -> 8 bits (halo {fused.halo})", flush=True)
t_fa = timed("lipasr_defence_apply, the chain in one launch", lambda: fused.apply(x, out=bufs[3]))
t_ca = timed("lipasr_defence_apply, three single-stage launches", composed_apply)
assert torch.equal(bufs[3].view(torch.int32), bufs[2].view(torch.int32))
t_fv = timed("lipasr_defence_vjp, the chain in one launch (recomputes the forward pass)", lambda: fused.vjp(x, g, out=gf))
t_cv = timed("lipasr_defence_vjp, three single-stage launches (inputs kept by the forward)", composed_vjp)
assert torch.equal(gf.view(torch.int32), gb[0].view(torch.int32))
print("each stage alone, apply / vjp:", flush=True)
for name, d in zip(("median 5", "low-pass 101 taps", "8 bits"), singles):
    timed(f"{name}: lipasr_defence_apply", lambda: d.apply(x, out=bufs[3]))
    timed(f"{name}: lipasr_defence_vjp", lambda: d.vjp(x, g, out=gf))
cap = AudioDefence([("median", 15), ("fir", np.ones(255, dtype=np.float32) / 255), ("fir", np.ones(245, dtype=np.float32) / 245), ("quantize", 4)])
print(f"the widest chain there is: median 15 -> 255 taps -> 245 taps -> 4 bits (halo {cap.halo})", flush=True)
timed("lipasr_defence_apply", lambda: cap.apply(x, out=bufs[3]))
timed("lipasr_defence_vjp", lambda: cap.vjp(x, g, out=gf))

model = T.get_model(max_batch=1024)
ex = MfccExtractor(16000, 16000, batch_max=1024)
clf = WaveformClassifier(model, 10, extractor=ex, utterance_length=44, domain="22k")
est = DefendedClassifier(clf, fused)
y = torch.eye(10, device=dev)[torch.arange(rows, device=dev) % 10].contiguous()
grad = torch.empty_like(x)
print(f"the classifier behind it: WaveformClassifier.loss_gradient_device over {rows} rows x {n} (extraction, the model's two passes, the MFCC backward pass)", flush=True)
t_c = timed("WaveformClassifier.loss_gradient_device", lambda: clf.loss_gradient_device(x, y, out=grad))
t_d = timed("DefendedClassifier.loss_gradient_device (chain)", lambda: est.loss_gradient_device(x, y, out=grad))
print(f"  fused {t_fa + t_fv:.3f} ms (apply {t_fa:.3f} + vjp {t_fv:.3f}) against composed {t_ca + t_cv:.3f} ms (apply {t_ca:.3f} + vjp {t_cv:.3f}): "
      f"{(t_ca + t_cv) / (t_fa + t_fv):.2f} x; against the classifier's {t_c:.3f} ms: {(t_fa + t_fv) / t_c:.2f} x; defended gradient {t_d:.3f} ms", flush=True)
ex.close()
