"""HIP-event timing of the psychoacoustic entry points at batch 64 x 22 050 samples (one second at 22 050 Hz, 40 frames): one
process, whole chip, medians over --iters calls after --warm warm-up calls (profiles/psycho_timing.txt).  lipasr_psy_prepare runs
once per clip batch, lipasr_psy_loss_grad on every stage-2 iteration of the imperceptible attack; beside them the MFCC backward
pass lipasr_mfcc_plan_vjp(flags=1) at the same batch and length, the kernel of the same structure (two 2048-point transforms per
frame pair) that each of those iterations also runs."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.psychoacoustic import PsychoacousticMasker

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--amp", type=float, default=1e-2)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, n, L = args.batch, 22050, 44
rng = np.random.default_rng(3)
t = np.arange(n) / 22050.0
x = np.stack([sum(rng.uniform(0.02, 0.2) * np.sin(2 * np.pi * rng.uniform(100, 9000) * t + rng.uniform(0, 6.28)) for _ in range(5))
              + 0.01 * rng.standard_normal(n) for _ in range(B)]).astype(np.float32)
x = torch.as_tensor(x).to(dev)
delta = torch.as_tensor((args.amp * rng.standard_normal((B, n))).astype(np.float32)).to(dev)
mk = PsychoacousticMasker(sample_rate=22050)
theta, mx = mk.prepare_device(x)
g = torch.empty_like(x)

def timed(name, fn):
    for _ in range(args.warm): fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
    ev[0].record()
    for i in range(args.iters):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    tt = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]) * 1e3
    print(f"{name:72s} median {np.median(tt):9.1f} us  min {tt.min():9.1f}  p90 {np.percentile(tt, 90):9.1f}", flush=True)
    return float(np.median(tt))

plan, st = mk._plan(n, B), N.stream_ptr()
loss = torch.empty(B, device=dev)
r = {}
r["prepare"] = timed("lipasr_psy_prepare (psd, finish, threshold)",
                     lambda: N.check(N.lib.lipasr_psy_prepare(plan, N.ptr(x), n, B, N.ptr(theta), N.ptr(mx), st)))
r["lg"] = timed(f"lipasr_psy_loss_grad (delta = {args.amp} x noise)",
                lambda: N.check(N.lib.lipasr_psy_loss_grad(plan, N.ptr(delta), n, B, N.ptr(theta), N.ptr(mx), N.ptr(loss), N.ptr(g), st)))
r["l"] = timed("lipasr_psy_loss_grad, g_delta = NULL (loss alone)",
               lambda: N.check(N.lib.lipasr_psy_loss_grad(plan, N.ptr(delta), n, B, N.ptr(theta), N.ptr(mx), N.ptr(loss), None, st)))
over = float((mk.loss_gradient_device(delta, theta, mx, need_grad=False)[0] > 0).float().mean())
ex = MfccExtractor(22050, n, batch_max=B)
gf = torch.as_tensor(rng.standard_normal((B, 20 * L)).astype(np.float32)).to(dev)
feat = ex.from_22k(x, L)
r["vjp"] = timed("lipasr_mfcc_plan_vjp(flags=1), domain 22k (db + stft_vjp + fold)", lambda: ex.vjp(x, gf, L, domain="22k", reuse_forward=True, out=g))
print(f"loss_grad / mfcc vjp: {r['lg'] / r['vjp']:.2f} x; rows with a positive loss: {100 * over:.0f}%")
mk.close(); ex.close()
