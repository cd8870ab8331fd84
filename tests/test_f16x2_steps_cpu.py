"""(no GPU) The swing of test_f16x2_steps_gpu.py is decisive, shown on the float64 oracle alone.

The oracle runs with every matrix-product operand rounded to two fp16 planes (numpy float16: hi = f16(x c), lo = f16(x c - hi), value
(hi + lo) / c) at the scales the design gives each kind of operand (f16x2_steps.TwoPlaneOperands).  The dz of every BatchNorm layer
takes 2^(14 - e) from its own maximum -- and, second, that scale divided by 2^S, which is what a step sees whose gradients are 2^S
times smaller than those of the step that left the scale behind.

  * at the design's scale every tensor of every case stays inside _fp32_bound (the rounding itself costs 0.4 % to 2.1 % of the bound);
  * at the stale scale at least one weight gradient of every case misses its bound tenfold or more;
  * S = 27 is the smallest such swing: at 26 the W_WIDE cases reach 6.8 times the bound only.

Figures (share of _fp32_bound; the cases on one problem share a figure):

  problem (cases)                                      design scale, worst tensor   stale by 2^27, worst dW   by 2^26
  W_SMALL batch 77  (chain-frag, exchange-frag)        0.0069 (dW1)                 30.1                      17.8
  W_LDS   batch 150 (chain-lds, exchange-ring-x1/ring) 0.021  (dW1)                 35.9                      19.6
  W_LDS   batch 300 (exchange-ring2)                   0.013  (dW0)                 31.9                      18.2
  W_WIDE  batch 100 (group-*, head-dw0-lds)            0.0040 (db0)                 15.3                       6.8

The swing moves the static scale 2^8 / 2^e of inv_batch along with the gradients, so it cannot see a GEMM that does not read the
maximum at all (a null sa_dyn / sb_dyn falls back to that scale).  The second problem per case moves the gradients against
inv_batch: gamma of the last BatchNorm layer times 2^-T (f16x2_steps.shrunk).  T = 19 is the smallest shift at which every dz at
the static scale puts a weight gradient at ten times its bound or more on every case's problem, the design's scales staying inside:

  problem             design scale, worst tensor   static scale, worst dW   at T - 1
  W_SMALL batch 77    0.0074                       339                      197
  W_LDS   batch 150   0.011                        1070                     482
  W_LDS   batch 300   0.018                        654                      385
  W_WIDE  batch 100   0.0032                       13.8                     8.6

These are estimates of what a stale or unread scale costs.  They are no model of the kernels' bits and no device value is compared
with them."""
import numpy as np

from f16x2_steps import S, STEP_CASES, T, two_plane, two_plane_errors


def test_two_plane_rounding_keeps_22_bits():
    """The rounding itself: 2^-22 relative while the low plane is a normal fp16 number, an absolute 2^-25 / c once it is not."""
    x = np.random.default_rng(0).uniform(0.25, 1.0, 4096)
    assert (np.abs(two_plane(x, 4096.0) - x) <= x * 2.0 ** -22).all()
    tiny = x * 2.0 ** -30
    assert (np.abs(two_plane(tiny, 4096.0) - tiny) <= 2.0 ** -25 / 4096.0).all()
    assert np.abs(two_plane(tiny, 4096.0) - tiny).max() > 2.0 ** -27 / 4096.0


def test_swing_is_large_enough_to_break_a_stale_scale():
    assert S <= 40
    print(f"\nswing S = {S}")
    least = {S: np.inf, S - 1: np.inf}
    for case in STEP_CASES:
        design = two_plane_errors(case, 0)
        stale = {s: max(v for k, v in two_plane_errors(case, s).items() if k.startswith("dW")) for s in least}
        worst = max(design, key=design.get)
        print(f"{case['id']}: design scale {design[worst]:.3g} of the bound ({worst}); stale by 2^{S}: {stale[S]:.3g}, by 2^{S - 1}: {stale[S - 1]:.3g} (worst dW)")
        assert all(v < 1.0 for v in design.values()), (case["id"], design)
        assert stale[S] >= 10.0, (case["id"], stale[S])
        for s in least:
            least[s] = min(least[s], stale[s])
    assert least[S - 1] < 10.0, "a smaller swing would do"


def test_gamma_shift_is_large_enough_to_break_an_unread_scale():
    print(f"\ngamma shift T = {T}")
    least = {T: np.inf, T - 1: np.inf}
    for case in STEP_CASES:
        design = two_plane_errors(case, shift=T)
        static = {t: max(v for k, v in two_plane_errors(case, static=True, shift=t).items() if k.startswith("dW")) for t in least}
        worst = max(design, key=design.get)
        print(f"{case['id']}: design scale {design[worst]:.3g} of the bound ({worst}); static scale at 2^-{T}: {static[T]:.3g}, at 2^-{T - 1}: {static[T - 1]:.3g} (worst dW)")
        assert all(v < 1.0 for v in design.values()), (case["id"], design)
        assert static[T] >= 10.0, (case["id"], static[T])
        for t in least:
            least[t] = min(least[t], static[t])
    assert least[T - 1] < 10.0, "a smaller shift would do"
