"""HIP-event timing of bound propagation at 1 024 rows on the 880 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 10 model: lipasr_mlp_bounds
without its backward pass (IBP: the prep kernel, five interval layers, the head) and with it (CROWN-IBP: five more products over
10 240 = rows x classes rows, the tail), and, on the same run, one predict_device pass over the same rows.  The questions the numbers
answer: what a certificate costs next to a forward pass, and what share of the fp32 matrix peak (157.3 TFLOP/s) the two tile kernels
reach; the FLOPs counted are the useful ones -- forward 3 x the five hidden products (W c, |W| r, |W| |c| from one read of W),
backward classes x the same five.  One process, whole chip, medians over --iters calls after --warm warm-up calls, repeated
--repeats times for the spread (profiles/bounds_timing.txt)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, train_constraints as T
from lipasr.attacks import TensorFlowV2Classifier
from lipasr import bounds as B

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=30); ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--rows", type=int, default=1024)
args = ap.parse_args()
dev = torch.device("cuda", 0)
PEAK = 157.3e12
print(f"library {os.path.relpath(N.LIB_PATH, ROOT)} version {N.lib.lipasr_version()}", flush=True)


def timed(name, fn, flop=None):
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
    rate = "" if flop is None else f"  {flop / med / 1e9:7.1f} TFLOP/s = {100 * flop / (med * 1e-3) / PEAK:4.1f} % of the fp32 matrix peak"
    print(f"  {name:64s} median {med:8.3f} ms  (medians of {args.repeats} runs: {min(meds):.3f} .. {max(meds):.3f}; last run min {t.min():.3f} "
          f"p90 {np.percentile(t, 90):.3f}){rate}", flush=True)
    return med


rows = args.rows
model = T.get_model(max_batch=rows)
w = model._widths
clf = TensorFlowV2Classifier(model=model, nb_classes=w[-1], input_shape=(w[0],))
rng = np.random.default_rng(0)
x = torch.as_tensor(rng.standard_normal((rows, w[0])).astype(np.float32)).to(dev)
eps = torch.full((rows,), 0.01, device=dev)
y = clf.own_labels_device(x).argmax(dim=1).to(torch.int32).contiguous()
ws = B._Workspace(model)
clip = (-float("inf"), float("inf"))
hidden = sum(2.0 * rows * a * b for a, b in zip(w[:-2], w[1:-1]))
print(f"{rows} rows on {' -> '.join(str(v) for v in w)}: forward {3 * hidden / 1e9:.1f} GFLOP (3 x the hidden products), backward "
      f"{w[-1] * hidden / 1e9:.1f} GFLOP ({w[-1]} x)", flush=True)
for norm in (float("inf"), 2.0):
    print(f"norm {norm}", flush=True)
    t_f = timed("lipasr_mlp_bounds, IBP only (forward: L + 1 launches)", lambda: B._margins(clf, x, eps, y, norm, clip, "ibp", ws), 3 * hidden)
    t_b = timed("lipasr_mlp_bounds, CROWN-IBP (forward + backward: 2 L + 1)", lambda: B._margins(clf, x, eps, y, norm, clip, "crown-ibp", ws))
    print(f"  the backward pass alone (difference of the two medians)          {t_b - t_f:8.3f} ms  "
          f"{w[-1] * hidden / (t_b - t_f) / 1e9:7.1f} TFLOP/s = {100 * w[-1] * hidden / ((t_b - t_f) * 1e-3) / PEAK:4.1f} % of the fp32 matrix peak", flush=True)
t_p = timed("predict_device over the same rows", lambda: clf.predict_device(x, logits=True))
print(f"  one certificate (norm 2, the last pair above): IBP {t_f / t_p:.1f} x, CROWN-IBP {t_b / t_p:.1f} x a forward pass of {t_p:.3f} ms", flush=True)
