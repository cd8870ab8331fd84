"""HIP-event timing of the MFCC backward pass with per-clip lengths (lipasr_mfcc_plan_vjp_ragged) against the one-length call
(lipasr_mfcc_plan_vjp) at batch 1024 x 16 000 samples: one process, whole chip, medians over --iters calls after --warm warm-up
calls (profiles/wave_vjp_ragged_timing.txt).  Every call reuses the forward, as the attacks do.

    python scratch/time_wave_vjp_ragged.py                 the one-length call, every clip full-length, lengths uniform in 4000..16000
    python scratch/time_wave_vjp_ragged.py --tree DIR      the one-length call alone, with the package and library of the checkout
                                                           at DIR: a build of the parent commit, timed in the same session on
                                                           the same machine, is the baseline
"""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200); ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--tree", default=None, help="another checkout (built) whose one-length call is timed instead")
args = ap.parse_args()
if args.tree:
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "asr-using-robust-nn_amd"))
from lipasr import _native as N
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.synth import synth_clips_fast

dev = torch.device("cuda", 0)
B, L = 1024, 44
waves, _ = synth_clips_fast(B, seed=7)
x = torch.as_tensor(waves).to(dev)
ex = MfccExtractor(16000, 16000, batch_max=B)
y22 = ex.resample(x)
g = torch.randn(B, 880, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
out22, outx, feat = torch.empty_like(y22), torch.empty_like(x), torch.empty(B, 880, device=dev)
print(f"library {N.LIB_PATH} version {N.lib.lipasr_version()}", flush=True)


def timed(name, fn):
    for _ in range(args.warm): fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
    ev[0].record()
    for i in range(args.iters):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    t = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]) * 1e3
    print(f"{name:64s} median {np.median(t):9.1f} us  mean {t.mean():9.1f}  min {t.min():9.1f}  p90 {np.percentile(t, 90):9.1f}", flush=True)
    return float(np.median(t))


r = {}
ex.from_22k(y22, L, out=feat)
r["u22"] = timed("vjp domain 22k, reuse_forward, one length", lambda: ex.vjp(y22, g, L, domain="22k", reuse_forward=True, out=out22))
ex(x, L, out=feat)
r["u0"] = timed("vjp domain input, reuse_forward, one length", lambda: ex.vjp(x, g, L, domain="input", reuse_forward=True, out=outx))
if not args.tree:
    full = torch.full((B,), 16000, dtype=torch.int32, device=dev)
    mixed = torch.as_tensor(np.random.default_rng(3).integers(4000, 16001, size=B).astype(np.int32)).to(dev)
    for name, lt in (("full", full), ("mixed", mixed)):
        what = "every clip full-length" if name == "full" else f"lengths uniform in 4000..16000 (mean {float(lt.float().mean()):.0f})"
        y = ex.resample(x, n_valid=lt)
        ex.from_22k(y, L, out=feat, n_valid=lt)
        r[name + "22"] = timed(f"vjp_ragged domain 22k, reuse_forward, {what}",
                               lambda: ex.vjp_ragged(y, g, lt, L, domain="22k", reuse_forward=True, out=out22))
        ex(x, L, out=feat, n_valid=lt)
        r[name + "0"] = timed(f"vjp_ragged domain input, reuse_forward, {what}",
                              lambda: ex.vjp_ragged(x, g, lt, L, domain="input", reuse_forward=True, out=outx))
    print(f"full-length ragged / one length: 22k {r['full22'] / r['u22']:.3f}, input {r['full0'] / r['u0']:.3f}; "
          f"mixed / full-length ragged: 22k {r['mixed22'] / r['full22']:.3f}, input {r['mixed0'] / r['full0']:.3f}")
