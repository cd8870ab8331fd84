"""TrainPipeline's schedule policy as a pure function of its arguments and the LIPASR_* variables (knobs.py): no torch, no native
library, no device.  The constructor turns the plan into streams; the fields marked "wish" need a stream that may fail to come
into being, and TrainPipeline.__init__ applies those conditions once."""
from dataclasses import dataclass
from typing import Optional

from . import knobs


@dataclass(frozen=True)
class Schedule:
    n_cu: int
    use_graph: bool
    mfcc_groups: Optional[int]  # the extraction's mask: the first k groups of 8 CUs (one CU of every XCD each); None: no partition
    classifier: str             # "rest": the groups the extraction does not have; "own_queue": every CU, a hardware queue of its own; "pool"
    gemm_tiles: Optional[int]   # "rest" only: the plan's LDS-tile threshold ...
    cu_budget: Optional[int]    # ... and the CUs its stream really has
    flags: bool                 # hand-offs by device flags (wish), else events
    wide: bool                  # an unmasked stream for extractions that find the classifier idle (wish)
    adam_signal: bool           # the Adam kernel raises "buffer free" (wish: needs the flags)

    @property
    def mfcc_cus(self):
        return None if self.mfcc_groups is None else 8 * self.mfcc_groups

    @property
    def train_cus(self):
        return self.cu_budget if self.classifier == "rest" else self.n_cu

    @property
    def classifier_groups(self):
        """The (first, end) groups of the classifier's mask, None on a pool stream."""
        if self.classifier == "pool":
            return None
        return (self.mfcc_groups, self.n_cu // 8) if self.classifier == "rest" else (0, (self.n_cu + 7) // 8)


def plan_schedule(*, n_cu, batch, compute_dtype="float32", pgd=False, custom_extractor=False, mfcc_cus="auto", train_cus="auto",
                  use_graph="auto", world=1, sync_bn=False, constraint="product", has_adam_signal=True):
    """The arguments are TrainPipeline's (pgd, custom_extractor as booleans; sync_bn as it holds, i.e. False on one device)."""
    # "auto": graphs for the long launch sequences (PGD, synchronized BatchNorm), plain launches for the 29-kernel step
    # (the measurements are in TrainPipeline's docstring)
    graph = bool(pgd or sync_bn) if use_graph == "auto" else bool(use_graph)
    # The classifier on the REST of the chip or on ALL of it: the caller's word, then LIPASR_TRAIN_CUS, then "rest" for the plain
    # step on the built-in MFCC plan.  PGD adversarial training is the other regime: the classifier's leg is ten times the MFCC's
    # and throughput-bound on its GEMMs, so it keeps every CU (PGD-20, batch 1024: 4.09 ms with 128 CUs for the MFCC and the
    # classifier everywhere; 4.14 / 4.25 with 64 / 32; on the rest of the chip only: 4.67 / 5.05 / 5.24 with 32 / 64 / 96)
    want = train_cus if train_cus != "auto" else (knobs.get("LIPASR_TRAIN_CUS") or ("all" if (custom_extractor or pgd) else "rest"))
    rest = want == "rest"
    if mfcc_cus == "auto":
        # The MFCC kernels are throughput kernels with thousands of workgroups; the classifier step is a chain of ~30 short
        # dependent kernels.  Sharing every CU, the chain's workgroups queue behind MFCC workgroups for LDS and wave slots.
        # measured at per-GPU batch 1024 on MI355X: 0.591 ms per step unmasked, 0.549 / 0.529 / 0.518 / 0.513 / 0.510 /
        # 0.506 / 0.532 / 0.528 with 240 / 224 / 208 / 192 / 176 / 160 / 144 / 128 CUs for the MFCC stream
        # (a heavier extractor wants a larger share: the 441/220 Speaker-recognition path measured 0.904 ms unmasked,
        # 0.865 / 0.826 / 0.811 with 160 / 192 / 224 CUs)
        # re-measured at the end of round 2 (after the STFT / GEMM changes): batch 1024: 0.540 / 0.505 / 0.489 / 0.520 ms
        # with 128 / 160 / 192 / 224 CUs; batch 512: 0.340 with 160, 0.349 with 192 -- the MFCC work grows with the
        # batch, the classifier's kernel chain hardly does, so the larger batch wants the larger share
        env = knobs.get("LIPASR_MFCC_CUS")
        if env is not None:
            mfcc_cus = env
        elif custom_extractor:
            mfcc_cus = (n_cu * 7) // 8
        elif rest and not (pgd and train_cus == "auto"):  # (PGD sent to the rest by LIPASR_TRAIN_CUS keeps the shared schedule's half)
            # round 3 (resampler on the fp16 matrix instruction, dual-FFT STFT kernel: the MFCC needs 155 us of the
            # whole chip instead of 240), 200-step runs, classifier stream on every CU: batch 1024: 0.499 / 0.460 / 0.481 /
            # 0.493 / 0.499 ms with 96 / 128 / 160 / 192 / 224 CUs; batch 512: 0.341 with 128, 0.353 with 160.
            # With the classifier's stream on the REST of the chip (train_cus="rest", 300-step runs, three repeats within
            # 0.002): batch 1024: 0.616 / 0.447 / 0.471 ms with 64 / 96 / 128 CUs for the MFCC (0.468 for the best shared
            # schedule, 0.517 with 96 CUs and the classifier everywhere); batch 512: 0.339 / 0.346 with 64 / 96 (0.347 shared)
            # after the grouped dW GEMM moved to LDS tiles: batch 1024: 0.614 / 0.431 / 0.453 with 64 / 96 / 128;
            # batch 2048: 0.871 / 0.679 with 96 / 128; batch 512: 0.337 with 64
            mfcc_cus = n_cu // 4 if batch <= 768 else ((n_cu * 3) // 8 if batch <= 1536 else n_cu // 2)
            # round 5: with the classifier's training GEMMs in arithmetic mode 2 (fp16 two-plane split, LDS-DMA ring) its
            # leg is 0.36 ms on 160 CUs and 0.37-0.38 on 128, so the extraction gets half the chip: batch 1024
            # 0.371 ms per step with 128 | 128 against 0.400 with 96 | 160 (200 steps, same box, interleaved)
            if compute_dtype == "float16x2" and 768 < batch <= 1536:
                mfcc_cus = n_cu // 2
        else:
            mfcc_cus = n_cu // 2
    # A classifier that keeps every CU (PGD, custom extractor, train_cus="all") does so on a stream with a FULL CU mask, NOT on a
    # stream of torch's pool: pool streams are multiplexed over GPU_MAX_HW_QUEUES (4) hardware queues, and once enough streams
    # exist in the process the training stream can land on the queue that carries the MFCC stream's kernels; its 440-node PGD
    # graph then waited behind them node by node: 13.0 ms per step instead of 4.1 as the fifth configuration of one process
    # (round 3's unexplained 3x; round 4: gone with GPU_MAX_HW_QUEUES=8).  A masked stream owns a hardware queue.
    own_queue = "own_queue" if knobs.get("LIPASR_TRAIN_OWN_QUEUE") == "1" else "pool"
    tiles = budget = None
    if not mfcc_cus or mfcc_cus >= n_cu:
        # no partition -- but a long dependent chain (the PGD graph: ~440 nodes) still must not sit on a pool stream
        groups, classifier = None, (own_queue if pgd else "pool")
    else:
        # Mask bits act in groups of 8 consecutive bits -- group g (bits 8g .. 8g+7) stands for CU g of every XCD -- so the share
        # is granted in steps of 8 CUs.  Pairs of settings 32 apart behaved alike (240/224, 208/192, 176/160, 144/128), so the
        # share is rounded down to a multiple of 32 CUs, which is what the hardware appears to grant; re-checked in round 3 with
        # the two disjoint partitions: 13, 14 and 15 groups leave the STFT kernel's time where 12 groups put it, 0.267 ms
        n_groups = max(1, n_cu // 8)
        groups = max(4, min((int(mfcc_cus) // 32) * 4, n_groups))
        classifier = "rest" if rest and groups < n_groups else own_queue
        if classifier == "rest":
            # on part of the chip the LDS-tiled GEMM pays from fewer tiles on (layer 2 forward, the dX GEMM into layer 2:
            # 128 tiles): -16 us on the classifier's graph at 160 CUs (PGD, which keeps every CU, loses 8 % with it)
            tiles = knobs.get("LIPASR_GEMM_TILES")
            tiles = 128 if tiles is None else tiles
            # the fused BatchNorm exchange spins until a column block's workgroups are all resident: the plan must know how
            # many CUs its stream really has (round 5)
            budget = 8 * (n_groups - groups)
    # Device flags instead of event pairs: 0.405 against 0.409 ms per step (round 4, batch 1024, same box back to back; config 5
    # 3.84 against 4.05-4.09 ms).  The default is events whenever ranks exchange gradients or BatchNorm sums (a rank sitting in a
    # collective while a peer checkpoints is a legitimate stall, and the flag kernels have never run beside an RCCL kernel:
    # no N > 1 run exists).  LIPASR_GPU_FLAGS=1 forces the flags on, 0 forces events (needed under tools that serialise kernels
    # across streams, e.g. rocprofv3 --pmc: a wait kernel would spin in front of the signal it waits for)
    flags = knobs.get("LIPASR_GPU_FLAGS")
    flags = (world == 1 and not sync_bn) if flags == "auto" else flags == "1"
    # When the classifier's stream is IDLE (the first step after a drained pipeline, a host-bound caller), the extraction does not
    # need to keep to its CU share: 0.19 instead of 0.39 ms for 1024 clips -- in a 20-step timed region that first extraction is
    # 0.02 ms per step (round 4)
    wide = groups is not None and not custom_extractor and knobs.get("LIPASR_WIDE_WHEN_IDLE") == "1"
    # "classifier done with buffer b" is true as soon as the step's forward / backward pass is: the eager single-device step with
    # the product constraint lets its Adam kernel raise free[b] when it starts instead of ending with a one-wavefront signal
    # launch, 2.5-5 us and a launch boundary on the critical stream.  Every other shape of a step keeps the trailing launch.
    adam = (flags and world == 1 and not sync_bn and not graph and constraint == "product" and bool(has_adam_signal)
            and knobs.get("LIPASR_ADAM_SIGNAL") == "1")
    return Schedule(n_cu, graph, groups, classifier, tiles, budget, flags, wide, adam)
