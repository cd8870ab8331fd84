"""HIP-event timing of the DolphinAttack entry points at batch 1024 x 16 000 samples: one process, whole chip, medians over
--iters calls after --warm warm-up calls, with the bytes each call moves through HBM (profiles/dolphin_timing.txt).  Under
rocprofv3 --kernel-trace --stats (a run of its own) the same script gives the per-kernel times."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N
from lipasr.dolphin import DolphinAttack
from lipasr.synth import synth_clips_fast

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--batch", type=int, default=1024)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, n = args.batch, 16000
waves, _ = synth_clips_fast(B, seed=7)
x = torch.as_tensor(waves).to(dev)
da = DolphinAttack(16000, n, B)
v, r = torch.empty_like(x), torch.empty_like(x)
s = torch.empty(B, 12 * n, device=dev)
st = N.stream_ptr()

def timed(name, nbytes, fn):
    for _ in range(args.warm): fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
    ev[0].record()
    for i in range(args.iters):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    t = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]) * 1e3
    med = float(np.median(t))
    print(f"{name:64s} median {med:9.1f} us  min {t.min():9.1f}  p90 {np.percentile(t, 90):9.1f}   {nbytes / 1e6:7.1f} MB  "
          f"{nbytes / med / 1e6:6.2f} TB/s  ({nbytes / 6e12 * 1e6:6.1f} us at 6 TB/s)", flush=True)
    return med

row = 4 * B * n  # bytes of one [B][16000] float32 array
t = {}
t["bp"] = timed("bandpass (wav -> voice)", 2 * row,
                lambda: N.check(N.lib.lipasr_dolphin_bandpass(da._plan, N.ptr(x), None, B, N.ptr(v), st)))
t["gen"] = timed("generate (band-pass, peaks, wav -> ultrasound)", 2 * row + 2 * row + row + 12 * row,
                 lambda: N.check(N.lib.lipasr_dolphin_generate(da._plan, N.ptr(x), None, B, N.ptr(s), None, st)))
t["rec"] = timed("record (ultrasound -> recorded clip)", 12 * row + row,
                 lambda: N.check(N.lib.lipasr_dolphin_record(da._plan, N.ptr(s), None, B, 1.0, 0.5, N.ptr(r), st)))
t["fused"] = timed("generate_recorded (band-pass, peaks, wav -> recorded clip)", 2 * row + 2 * row + 2 * row,
                   lambda: N.check(N.lib.lipasr_dolphin_generate_recorded(da._plan, N.ptr(x), None, B, 1.0, 0.5, N.ptr(r), st)))
print(f"generate + record {t['gen'] + t['rec']:.1f} us against generate_recorded {t['fused']:.1f} us: "
      f"{(t['gen'] + t['rec']) / t['fused']:.2f} x; without the shared band-pass: "
      f"{t['gen'] + t['rec'] - t['bp']:.1f} against {t['fused'] - t['bp']:.1f} us")
da.close()
