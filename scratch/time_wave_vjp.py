"""HIP-event timing of the MFCC backward pass (lipasr_mfcc_plan_vjp) and of one PGD iteration over audio at batch 1024 x 16 000
samples: one process, whole chip, medians over --iters calls after --warm warm-up calls (profiles/wave_vjp_timing.txt)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
from lipasr import _native as N, attacks as A
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.synth import synth_clips_fast
from helpers import build_model
from oracle import mlp_ref as P

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=200); ap.add_argument("--warm", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, L = 1024, 44
waves, labels = synth_clips_fast(B, seed=7)
x = torch.as_tensor(waves).to(dev)
ex = MfccExtractor(16000, 16000, batch_max=B)
y22 = ex.resample(x)
g = torch.randn(B, 880, device=dev)
gy = torch.randn(B, ex.n_y, device=dev)
out22, outx, feat = torch.empty_like(y22), torch.empty_like(x), torch.empty(B, 880, device=dev)
m = build_model(P.vd_unconstrained_spec(), max_batch=B)
yl = torch.zeros(B, 10, device=dev); yl[torch.arange(B), torch.as_tensor(labels.astype(np.int64)).to(dev)] = 1

def timed(name, fn):
    for _ in range(args.warm): fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
    ev[0].record()
    for i in range(args.iters):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    t = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]) * 1e3
    print(f"{name:58s} median {np.median(t):9.1f} us  mean {t.mean():9.1f}  min {t.min():9.1f}  p90 {np.percentile(t, 90):9.1f}", flush=True)
    return float(np.median(t))

r = {}
r["fwd22"] = timed("forward from_22k (STFT+mel+dB, DCT)", lambda: ex.from_22k(y22, L, out=feat))
r["fwd"] = timed("forward extract (resample, STFT+mel+dB, DCT)", lambda: ex(x, L, out=feat))
r["res"] = timed("forward resample alone", lambda: ex.resample(x, out=y22))
ex.from_22k(y22, L, out=feat)
r["vjp22_reuse"] = timed("vjp domain 22k, reuse_forward (STFT re-run + db + stft_vjp + fold)", lambda: ex.vjp(y22, g, L, domain="22k", reuse_forward=True, out=out22))
r["vjp22"] = timed("vjp domain 22k, forward re-run", lambda: ex.vjp(y22, g, L, domain="22k", out=out22))
r["rvjp"] = timed("resample_vjp alone", lambda: ex.resample_vjp(gy, out=outx))
ex(x, L, out=feat)
r["vjp0_reuse"] = timed("vjp domain input, reuse_forward (d_y reused; + resample_vjp)", lambda: ex.vjp(x, g, L, domain="input", reuse_forward=True, out=outx))
r["vjp0"] = timed("vjp domain input, forward re-run", lambda: ex.vjp(x, g, L, domain="input", out=outx))
# a plan whose forward is stft_mel2_kernel (stage-mask bit 256): the one 2048/512 forward whose tile flags bit 0 reuses
ex.set(0, 256)
r["fwd22_m"] = timed("mask 256: forward from_22k (stft_mel2_kernel, DCT)", lambda: ex.from_22k(y22, L, out=feat))
ex.from_22k(y22, L, out=feat)
r["vjp22_reuse_m"] = timed("mask 256: vjp domain 22k, reuse_forward (tile reused)", lambda: ex.vjp(y22, g, L, domain="22k", reuse_forward=True, out=out22))
ex(x, L, out=feat)
r["vjp0_reuse_m"] = timed("mask 256: vjp domain input, reuse_forward (tile reused)", lambda: ex.vjp(x, g, L, domain="input", reuse_forward=True, out=outx))
ex.set(0, 0)
h = N.get_handle(0)
for dom, x0 in (("22k", y22.clone()), ("input", x.clone())):
    clf = A.WaveformClassifier(m, 10, extractor=ex, utterance_length=L, domain=dom)
    xa, gg = x0.clone(), torch.empty_like(x0)
    def it():
        clf.loss_gradient_device(xa, yl, out=gg)
        N.check(N.lib.lipasr_lp_step(h.h, N.ptr(xa), N.ptr(x0), N.ptr(gg), B, xa.shape[1], float("inf"), 0.0025, 0.01, N.stream_ptr()))
        xa.clamp_(-1.0, 1.0)
    r["pgd_" + dom] = timed(f"one PGD-linf iteration over audio, domain {dom}", it)
print(f"backward/forward, 22k domain: {r['vjp22_reuse'] / r['fwd22']:.2f}; input domain: {r['vjp0_reuse'] / r['fwd']:.2f}")
