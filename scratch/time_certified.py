"""lipasr_timer_* timing of IBP certified training on the 880 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 10 model in exact fp32 at batch
1024: ms per certified step (Model.train_on_batch under IBPCrossentropy at its final eps and kappa) next to ms per plain step of the
same model, and the two native calls a certified step adds, each on its own: lipasr_mlp_bounds (IBP only, boxes kept) and
lipasr_mlp_bounds_grad.  --steps timed steps after --warm warm-up steps, --repeats times for the spread
(profiles/certified_timing.txt; the per-kernel split there comes from the same script under a kernel trace)."""
import sys, os, argparse, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, train_constraints as T
from lipasr.bounds import IBPCrossentropy
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
