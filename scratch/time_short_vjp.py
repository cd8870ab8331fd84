"""HIP-event timing of the short-window MFCC backward pass (lipasr_mfcc_plan_vjp_short, n_fft = 441, hop 220), of one loss_gradient
and one PGD iteration over [64, 22050] windows -- the Speaker-recognition batch -- and of the forward stft_mel stage from
profile_begin / profile_end: one process, whole chip, medians over --iters calls after --warm warm-up calls."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
from lipasr import _native as N, speaker_recognition as S
from helpers import build_model, load_params
from oracle import mlp_ref as P

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=200); ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B = args.batch
rng = np.random.default_rng(7)
t = np.arange(22050) / 22050.0
w = np.stack([0.3 * np.sin(2 * np.pi * (200.0 + 37.0 * i) * t * (1 + 0.2 * t)) + 0.02 * rng.standard_normal(22050) for i in range(B)]).astype(np.float32)
x = torch.as_tensor(w).to(dev)
spec = P.sr_unconstrained_spec()
m = build_model(spec, max_batch=B)
load_params(m, P.init_params(spec, seed=3, nonneg_init=False))
ex = S.WindowMfcc(batch_max=B)
g = torch.randn(B, 2020, device=dev)
feat, out = torch.empty(B, 2020, device=dev), torch.empty_like(x)
yl = torch.zeros(B, 20, device=dev); yl[torch.arange(B), torch.arange(B) % 20] = 1

def timed(name, fn):
    for _ in range(args.warm): fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
    ev[0].record()
    for i in range(args.iters):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    t = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]) * 1e3
    print(f"{name:62s} median {np.median(t):9.1f} us  mean {t.mean():9.1f}  min {t.min():9.1f}  p90 {np.percentile(t, 90):9.1f}", flush=True)
    return float(np.median(t))

print(f"library {N.LIB_PATH} version {N.lib.lipasr_version()} batch {B}", flush=True)
r = {}
r["fwd"] = timed("forward (dft_mel + DCT)", lambda: ex(x, out=feat))
for _ in range(args.warm): ex(x, out=feat)
ex.profile_begin(args.iters)
for _ in range(args.iters): ex._ex(x, 101, out=feat)  # the whole-extraction entry fills the profile slots (identity resampler: a copy)
prof, n = ex.profile_end()
print(f"forward stages from profile_begin/profile_end over {n} extractions: " + ", ".join(f"{k} {1e3 * v:.1f} us" for k, v in prof.items()), flush=True)
ex(x, out=feat)
r["vjp_reuse"] = timed("vjp_short, reuse_forward (db + dft_vjp + fold)", lambda: ex.vjp(x, g, reuse_forward=True, out=out))
r["vjp"] = timed("vjp_short, forward re-run", lambda: ex.vjp(x, g, out=out))
clf = S.waveform_classifier(m)
gg = torch.empty_like(x)
r["lossgrad"] = timed("loss_gradient_device (features, mlp_input_grad, vjp_short)", lambda: clf.loss_gradient_device(x, yl, out=gg))
h = N.get_handle(0)
xa = x.clone()
def it():
    clf.loss_gradient_device(xa, yl, out=gg)
    N.check(N.lib.lipasr_lp_step(h.h, N.ptr(xa), N.ptr(x), N.ptr(gg), B, xa.shape[1], float("inf"), 0.0025, 0.01, N.stream_ptr()))
    xa.clamp_(-1.0, 1.0)
r["pgd"] = timed("one PGD-linf iteration over the windows", it)
print(f"backward (reuse_forward) : forward stft_mel stage = {r['vjp_reuse'] / (1e3 * prof['stft_mel']):.2f}; : forward call = {r['vjp_reuse'] / r['fwd']:.2f}")
