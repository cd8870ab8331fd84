"""HIP-event timing of the over-the-air channel at the shape an EOT attack runs it: 64 clips x 16 rooms = 1 024 rows of 22 050
samples, 2 048 and 512 taps -- lipasr_room_apply, lipasr_room_vjp -- and, on the same run, one WaveformClassifier.loss_gradient_device
pass over the 1 024 rows (domain "22k"), which is what the channel sits in front of.  The question the numbers answer: what the
channel costs next to the classifier's two passes, and what share of the fp32 matrix peak (157.3 TFLOP/s) its kernels reach; the
FLOPs counted are the useful ones, 2 x rows x n x taps less the taps that fall before the clip's start.  One process, whole chip,
medians over --iters calls after --warm warm-up calls, repeated --repeats times for the spread (profiles/room_timing.txt)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, train_constraints as T
from lipasr.attacks import WaveformClassifier
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.room import RoomChannel, synthetic_rirs

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=30); ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
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


clips, rooms, n = 64, 16, 22050
rng = np.random.default_rng(0)
x = torch.as_tensor(rng.uniform(-0.5, 0.5, (clips, n)).astype(np.float32)).to(dev)
g = torch.as_tensor(rng.uniform(-1, 1, (clips * rooms, n)).astype(np.float32)).to(dev)
out, gx = torch.empty(clips * rooms, n, device=dev), torch.empty(clips, n, device=dev)
times = {}
for taps in (2048, 512):
    ch = RoomChannel(synthetic_rirs(rooms, taps=taps, seed=1))
    flop = 2.0 * clips * rooms * (n * taps - taps * (taps - 1) / 2.0)  # output t has min(t + 1, taps) taps
    print(f"{clips} clips x {rooms} rooms = {clips * rooms} rows x {n}, {taps} taps: {flop / 1e9:.1f} GFLOP per direction", flush=True)
    times[taps] = (timed("lipasr_room_apply", lambda: ch.apply(x, out=out), flop),
                   timed("lipasr_room_vjp (the 16 rooms summed)", lambda: ch.vjp(g, scale=1.0 / rooms, out=gx), flop))

model = T.get_model(max_batch=1024)
ex = MfccExtractor(16000, 16000, batch_max=1024)
clf = WaveformClassifier(model, 10, extractor=ex, utterance_length=44, domain="22k")
y = torch.eye(10, device=dev)[torch.arange(clips * rooms, device=dev) % 10].contiguous()
ch = RoomChannel(synthetic_rirs(rooms, taps=2048, seed=1))
rows = ch.apply(x)
grad = torch.empty_like(rows)
print(f"the classifier behind it: WaveformClassifier.loss_gradient_device over {clips * rooms} rows x {n} (extraction, the model's two passes, the MFCC backward pass)", flush=True)
t_c = timed("WaveformClassifier.loss_gradient_device", lambda: clf.loss_gradient_device(rows, y, out=grad))
for taps, (t_a, t_v) in times.items():
    print(f"  {taps} taps: channel {t_a + t_v:.3f} ms (apply {t_a:.3f} + vjp {t_v:.3f}) against the classifier's {t_c:.3f} ms: {(t_a + t_v) / t_c:.2f} x", flush=True)
ex.close()
