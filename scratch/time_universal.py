"""HIP-event timing of the four universal-perturbation kernels at the workload's shapes -- 1024 x 22 050 samples with P = 22 050 and
1024 x 880 features with P = 880, with and without drawn shifts, plus a looping snippet (P = 4000 < n) and the default minibatch of
32 rows -- beside a torch copy of the same bytes and the estimator's gradient call (its two passes) that a minibatch also pays.
lipasr_universal_reduce's bytes are what the algorithm needs: the gradient rows read once plus the fp64 partials written; its rate
is set against the 6.29 TB/s a float4 copy reaches on the MI355X.  The operands rotate over a pool of buffers larger than the
256 MB last-level cache, so that no call finds its rows there.  One process, whole chip; a figure is the time between two events
around --iters back-to-back calls divided by --iters, median (min .. max) of five such windows after --warm warm-up calls
(profiles/universal_timing.txt).  Calls shorter than about 9 us are bounded by the host's ctypes call, not by the kernel."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "asr-using-robust-nn_amd")]
import numpy as np, torch
from lipasr import _native as N, keras as K, train_constraints as T
from lipasr.attacks import TensorFlowV2Classifier, WaveformClassifier
from lipasr.extract_features_construct_dataset import MfccExtractor
from lipasr.universal import universal_apply, universal_reduce, universal_shifts, universal_step

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=50); ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--rows", type=int, default=1024)
args = ap.parse_args()
HBM = 6.29  # TB/s, float4 copy
print(f"library {os.path.relpath(N.LIB_PATH, ROOT)} version {N.lib.lipasr_version()} on {torch.cuda.get_device_name(0)}", flush=True)


def timed(fn, iters=None, warm=None):
    iters, warm = iters or args.iters, args.warm if warm is None else warm
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(5):
        a.record()
        for _ in range(iters): fn()
        b.record(); torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / iters * 1e3)
    return float(np.median(t)), f"{np.median(t):8.1f} us ({min(t):.1f} .. {max(t):.1f})"


def kernels(B, n, P, shift):
    print(f"{B} x {n}, P = {P}, {'drawn shifts' if shift else 'no shifts'}", flush=True)
    pool = [torch.randn(B, n, device="cuda") for _ in range(max(1, min(8, int(600e6 // (B * n * 4)))))]
    out, noise = torch.empty_like(pool[0]), torch.zeros(P, device="cuda")
    offs = universal_shifts(B, P, 0, 1) if shift else None
    groups = (B + N.UNIVERSAL_GROUP - 1) // N.UNIVERSAL_GROUP
    sums = torch.empty(groups, P, dtype=torch.float64, device="cuda")
    k = [0]

    def nxt():
        k[0] += 1
        return pool[k[0] % len(pool)]

    iters = args.iters if B * n > 1e6 else 4 * args.iters
    by = B * n * 4 + groups * P * 8
    us, s = timed(lambda: universal_reduce(nxt(), P, offs=offs, sums=sums), iters)
    print(f"  lipasr_universal_reduce  {s}  {by / 1e6:6.1f} MB  {by / us / 1e6:5.2f} TB/s = {100 * by / us / 1e6 / HBM:3.0f} % of {HBM} TB/s  (pool of {len(pool)})", flush=True)
    by = 2 * B * n * 4
    us, s = timed(lambda: universal_apply(nxt(), noise, offs=offs, out=out), iters)
    print(f"  lipasr_universal_apply   {s}  {by / 1e6:6.1f} MB  {by / us / 1e6:5.2f} TB/s", flush=True)
    us, s = timed(lambda: out.copy_(nxt()), iters)
    print(f"  torch copy, same bytes   {s}  {by / 1e6:6.1f} MB  {by / us / 1e6:5.2f} TB/s", flush=True)
    universal_reduce(pool[0], P, offs=offs, sums=sums)
    for norm in (np.inf, 2):
        _, s = timed(lambda: universal_step(noise, sums, norm, 0.01, 0.1), 4 * args.iters)
        print(f"  lipasr_universal_step, norm {str(norm):>3}, {groups:2d} groups  {s}", flush=True)
    o = torch.empty(B, dtype=torch.int32, device="cuda")
    _, s = timed(lambda: universal_shifts(B, P, 3, 1, out=o), 4 * args.iters)
    print(f"  lipasr_universal_shifts  {s}", flush=True)


B = args.rows
for shape in ((B, 22050, 22050, False), (B, 22050, 22050, True), (B, 880, 880, False), (B, 880, 880, True), (B, 22050, 4000, True),
              (32, 22050, 22050, True), (32, 880, 880, True)):
    kernels(*shape)

K.reset_layer_names()
m = T.get_model_unconstrained(max_batch=B)
m.compile(optimizer="adam", loss=K.CategoricalCrossentropy(), metrics=["accuracy"])
clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
ex = MfccExtractor(16000, 16000, batch_max=B)
wclf = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
y = torch.eye(10, device="cuda")[torch.randint(0, 10, (B,), device="cuda")].contiguous()
print("the estimator's two passes: loss_gradient_device", flush=True)
for name, est, n, scale in (("TensorFlowV2Classifier", clf, 880, 1.0), ("WaveformClassifier, domain 22k", wclf, 22050, 0.1)):
    for rows in (32, B):
        x = (scale * torch.randn(rows, n, device="cuda")).contiguous()
        g = torch.empty_like(x)
        _, s = timed(lambda: est.loss_gradient_device(x, y[:rows], out=g), 20, 3)
        print(f"  {name:32s} {rows:5d} x {n:5d}  {s}", flush=True)
ex.close()
