"""HIP-event timing of the time-warp operator at the shape a worst-of-grid query runs it: 128 clips x 27 candidates = 3 456 rows of
22 050 samples -- lipasr_warp_apply -- and, on the same run, WaveformClassifier.predict_device over the same 3 456 rows (domain
"22k"), which is what the operator feeds, and lipasr_warp_param_vjp at the refinement's shape (128 rows, K = 1) and at the grid's.
Next to each: the bytes the launch writes over its time against the HBM rate (8 TB/s), and the tap rate (rows x n x 32 taps, each
one LDS table read and two fmaf).  One process, whole chip, medians over --iters calls after --warm warm-up calls, repeated
--repeats times for the spread (profiles/warp_timing.txt)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, train_constraints as T
from lipasr.attacks import WaveformClassifier
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.warp import candidate_grid, warp_apply, warp_param_vjp

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
HBM = 8.0e12
print(f"library {os.path.relpath(N.LIB_PATH, ROOT)} version {N.lib.lipasr_version()} on {torch.cuda.get_device_name(0)}", flush=True)


def timed(name, fn, bytes_written=None, taps=None):
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
    extra = ""
    if bytes_written is not None:
        extra += f"  writes {bytes_written / 1e6:.0f} MB: {bytes_written / (med * 1e-3) / 1e12:.2f} TB/s = {100 * bytes_written / (med * 1e-3) / HBM:.1f} % of HBM"
    if taps is not None:
        extra += f"  {taps / (med * 1e-3) / 1e12:.2f} T taps/s"
    print(f"  {name:58s} median {med:8.3f} ms  (medians of {args.repeats} runs: {min(meds):.3f} .. {max(meds):.3f}; last run min {t.min():.3f} "
          f"p90 {np.percentile(t, 90):.3f}){extra}", flush=True)
    return med


clips, n = 128, 22050
rng = np.random.default_rng(0)
x = torch.as_tensor(rng.uniform(-0.5, 0.5, (clips, n)).astype(np.float32)).to(dev)
times = {}
for label, grid in (("27 = 3 delays x 3 rates x 3 gains (+-10 ms, 1.07, 3 dB)", candidate_grid(220.5, 1.07, 3.0, counts=(3, 3, 3))),
                    ("27 delays, rate 1 (+-10 ms)", candidate_grid(220.5, counts=(27, 1, 1)))):
    K = len(grid)
    params = torch.as_tensor(np.tile(grid, (clips, 1))).to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty(clips * K, n, device=dev)
    g = torch.as_tensor(rng.uniform(-1, 1, (clips * K, n)).astype(np.float32)).to(dev)
    print(f"{clips} clips x {K} candidates = {clips * K} rows x {n}: {label}", flush=True)
    times[label] = timed("lipasr_warp_apply", lambda: warp_apply(x, params, K, out=out), clips * K * n * 4, clips * K * n * 32)
    timed("lipasr_warp_param_vjp (every row of the grid)", lambda: warp_param_vjp(x, g, params, K), None, clips * K * n * 32)
p1 = torch.as_tensor(np.tile(candidate_grid(220.5, 1.07, 3.0, counts=(3, 3, 3))[5:6], (clips, 1))).to(device=dev, dtype=torch.float32).contiguous()
g1 = torch.as_tensor(rng.uniform(-1, 1, (clips, n)).astype(np.float32)).to(dev)
print(f"the refinement's shape: {clips} rows x {n}, K = 1", flush=True)
timed("lipasr_warp_apply", lambda: warp_apply(x, p1, 1), clips * n * 4, clips * n * 32)
timed("lipasr_warp_param_vjp", lambda: warp_param_vjp(x, g1, p1, 1), None, clips * n * 32)

model = T.get_model(max_batch=1024)
ex = MfccExtractor(16000, 16000, batch_max=1024)
clf = WaveformClassifier(model, 10, extractor=ex, utterance_length=44, domain="22k")
rows = warp_apply(x, params, 27)
print(f"what it feeds: WaveformClassifier.predict_device(logits=True) over {rows.shape[0]} rows x {n} (extraction and the model's forward pass)", flush=True)
t_c = timed("WaveformClassifier.predict_device", lambda: clf.predict_device(rows, logits=True))
for label, t_a in times.items():
    print(f"  {label}: warp_apply {t_a:.3f} ms against the forward pass's {t_c:.3f} ms: {t_a / t_c:.2f} x", flush=True)
ex.close()
