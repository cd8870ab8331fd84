"""lipasr_timer_* timing of IBP certified training on the 880 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 10 model in exact fp32 at batch
1024: ms per certified step (Model.train_on_batch under IBPCrossentropy at its final eps and kappa) next to ms per plain step of the
same model, and the two native calls a certified step adds, each on its own: lipasr_mlp_bounds (IBP only, boxes kept) and
lipasr_mlp_bounds_grad.  Then the same for CROWN-IBP certified training (CrownIBPCrossentropy at beta 1): its step, lipasr_mlp_bounds
with margin_crown, and lipasr_mlp_bounds_crown_grad alone, with the FLOP of its GEMM-shaped kernels.  --steps timed steps after
--warm warm-up steps, --repeats times for the spread (profiles/certified_timing.txt, profiles/crown_ibp_timing.txt; the per-kernel
split there comes from the same script under a kernel trace)."""
import sys, os, argparse, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, train_constraints as T
from lipasr.bounds import CrownIBPCrossentropy, IBPCrossentropy
from lipasr.keras import CategoricalCrossentropy, to_categorical

ap = argparse.ArgumentParser(); ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--batch", type=int, default=1024)
args = ap.parse_args()
dev = torch.device("cuda", 0)
print(f"library {os.path.relpath(N.LIB_PATH, ROOT)} version {N.lib.lipasr_version()} on {torch.cuda.get_device_name(0)}", flush=True)
h = N.get_handle(0)
tid = C.c_int()
N.check(N.lib.lipasr_timer_create(h.h, C.byref(tid)))


def timed(name, fn):
    per = []
    for _ in range(args.repeats):
        for _ in range(args.warm): fn()
        torch.cuda.synchronize()
        N.check(N.lib.lipasr_timer_start(h.h, tid.value, N.stream_ptr()))
        for _ in range(args.steps): fn()
        N.check(N.lib.lipasr_timer_stop(h.h, tid.value, N.stream_ptr()))
        torch.cuda.synchronize()
        ms = C.c_float()
        N.check(N.lib.lipasr_timer_elapsed_ms(h.h, tid.value, C.byref(ms)))
        per.append(ms.value / args.steps)
    print(f"  {name:58s} {np.median(per):8.3f} ms per call  ({args.steps} calls after {args.warm}; {args.repeats} runs: {min(per):.3f} .. {max(per):.3f})", flush=True)
    return float(np.median(per))


B = args.batch
rng = np.random.default_rng(0)
x = torch.as_tensor(rng.standard_normal((B, 880)).astype(np.float32)).to(dev)
y = torch.as_tensor(to_categorical(rng.integers(0, 10, B), 10)).to(dev)
models = {}
for name, loss in (("plain", CategoricalCrossentropy()), ("certified", IBPCrossentropy(0.01, kappa=0.5))):
    m = T.get_model(max_batch=B, compute_dtype="float32")
    m.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
    if name == "certified":
        loss.step = 1  # past the one-step ramp
    models[name] = m
w = models["plain"]._widths
hidden = sum(2.0 * B * a * b for a, b in zip(w[:-2], w[1:-1]))
print(f"batch {B} on {' -> '.join(str(v) for v in w)}: one hidden product is {hidden / 1e9:.2f} GFLOP over the five hidden layers", flush=True)
t_plain = timed("plain step (train_on_batch, CategoricalCrossentropy)", lambda: models["plain"].train_on_batch(x, y))
t_cert = timed("certified step (train_on_batch, IBPCrossentropy)", lambda: models["certified"].train_on_batch(x, y))
m = models["certified"]
loss = m._loss
buf = loss._buffers(m)
yt = y.argmax(dim=1).to(torch.int32)
buf["eps"].fill_(0.01)
args3 = (m._plan, N.ptr(m._params), N.ptr(m._bnstate))
fwd = lambda: N.check(N.lib.lipasr_mlp_bounds(*args3, N.ptr(x), N.ptr(buf["eps"]), float("inf"), -float("inf"), float("inf"), N.ptr(yt), B,
                                              N.ptr(buf["ws"]), buf["ws"].numel(), N.ptr(buf["margin"]), None, None, N.ptr(buf["lo"]),
                                              N.ptr(buf["hi"]), N.stream_ptr()))
bwd = lambda: N.check(N.lib.lipasr_mlp_bounds_grad(*args3, N.ptr(buf["margin"]), N.ptr(buf["lo"]), N.ptr(buf["hi"]), N.ptr(yt), B,
                                                   N.ptr(buf["ws_grad"]), buf["ws_grad"].numel(), 1.0, 0.5 / B, N.ptr(m._grads),
                                                   N.ptr(buf["rows"]), N.stream_ptr()))
t_f = timed("lipasr_mlp_bounds alone (IBP only, boxes kept)", fwd)
t_b = timed("lipasr_mlp_bounds_grad alone", bwd)
print(f"  certified / plain {t_cert / t_plain:.2f} x; the bound path (certified - plain) {t_cert - t_plain:.3f} ms, of which the interval forward "
      f"{t_f:.3f} ms ({100 * t_f / t_cert:.0f} % of the certified step) and its backward {t_b:.3f} ms ({100 * t_b / t_cert:.0f} %)", flush=True)
print(f"  products: the plain step has 3 per hidden layer, the bound path 7 (forward W c, |W| r, |W| |c|; weight gradient c^T gc, r^T gr; "
      f"back gc W^T, gr |W|^T; the first layer has no back product): counted ratio {(7 * hidden - 2 * 2.0 * B * w[0] * w[1]) / (3 * hidden - 2.0 * B * w[0] * w[1]):.2f}, "
      f"measured {(t_cert - t_plain) / t_plain:.2f}", flush=True)

# ---------------------------------------------------------------------------------------------------------------- CROWN-IBP
cm = T.get_model(max_batch=B, compute_dtype="float32")
closs = CrownIBPCrossentropy(0.01, kappa=0.5, beta_start=1.0, beta_end=1.0)
cm.compile(optimizer="adam", loss=closs, metrics=["accuracy"])
closs.step = 1
t_crown = timed("CROWN-IBP step (train_on_batch, CrownIBPCrossentropy, beta 1)", lambda: cm.train_on_batch(x, y))
cbuf = closs._crown_buffers(cm)
cbuf["eps"].fill_(0.01)
cargs = (cm._plan, N.ptr(cm._params), N.ptr(cm._bnstate))
cfwd = lambda: N.check(N.lib.lipasr_mlp_bounds(*cargs, N.ptr(x), N.ptr(cbuf["eps"]), float("inf"), -float("inf"), float("inf"), N.ptr(yt), B,
                                               N.ptr(cbuf["ws"]), cbuf["ws"].numel(), N.ptr(cbuf["margin"]), N.ptr(cbuf["margin_crown"]), None,
                                               N.ptr(cbuf["lo"]), N.ptr(cbuf["hi"]), N.stream_ptr()))
cbwd = lambda beta: N.check(N.lib.lipasr_mlp_bounds_crown_grad(*cargs, N.ptr(cbuf["margin"]), N.ptr(cbuf["margin_crown"]), N.ptr(cbuf["lo"]),
                                                               N.ptr(cbuf["hi"]), N.ptr(yt), B, beta, N.ptr(cbuf["ws_crown"]),
                                                               cbuf["ws_crown"].numel(), 1.0, 0.5 / B, N.ptr(cm._grads), N.ptr(cbuf["rows"]),
                                                               N.stream_ptr()))
t_cf = timed("lipasr_mlp_bounds alone (with margin_crown, boxes kept)", cfwd)
t_cb = timed("lipasr_mlp_bounds_crown_grad alone, beta 1", lambda: cbwd(1.0))
t_c0 = timed("lipasr_mlp_bounds_crown_grad alone, beta 0", lambda: cbwd(0.0))
M = B * w[-1]
mflop = sum(2.0 * M * a * b for a, b in zip(w[:-2], w[1:-1]))
print(f"  CROWN-IBP / plain {t_crown / t_plain:.2f} x, / IBP certified {t_crown / t_cert:.2f} x; workspace of the new call "
      f"{cbuf['ws_crown'].numel() * 4 / 2 ** 20:.0f} MiB", flush=True)
print(f"  M = batch x classes = {M}: one product over the five hidden layers is {mflop / 1e9:.2f} GFLOP; the new call makes three (chain, "
      f"adjoint, weight gradient) next to the interval sweep: {3 * mflop / 1e9:.1f} GFLOP in {t_cb - t_c0:.3f} ms = "
      f"{3 * mflop / (t_cb - t_c0) / 1e9:.1f} TFLOP/s with everything else in that time", flush=True)
for l, (a, b) in enumerate(zip(w[:-2], w[1:-1])):
    print(f"    layer {l + 1}: {a} x {b}, {2.0 * M * a * b / 1e9:.3f} GFLOP per product", flush=True)
