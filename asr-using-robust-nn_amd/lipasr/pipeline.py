"""The end-to-end training step of BASELINE configs 3-5 as one stream-ordered native sequence:

    waveform batch --K1--> MFCC --A2 affine (fused)--> [PGD-k on the features, K2+K4]
        --K2--> fwd/bwd --(RCCL all-reduce)--> K5 Adam+NonNeg --K3--> Lipschitz projection

Everything after the MFCC reads and writes fixed device buffers, so it is captured once per batch size
into HIP graphs (lipasr_graph_*) and replayed; Adam's step count, the dropout counter and all
projection scalars live in device memory, so a replay needs no host value.  The MFCC kernels read the
resident waveform pool in place and are launched eagerly (3 launches per step).

Two HIP streams: the MFCC of batch i+1 (VALU/LDS-bound kernels) runs on its own stream while the
classifier step of batch i (many short MFMA / latency-bound kernels) runs on the training stream; the
feature and label buffers are double-buffered and handoff.py carries the two dependencies
(features ready -> train; train done with a buffer -> MFCC may overwrite it).  Which CUs and queues
the two streams get is schedule.py's decision.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N, knobs
from .attacks import _norm_value
from .extract_features_construct_dataset import MfccExtractor
from .handoff import EventHandoff, FlagHandoff
from .parallel import DataParallel
from .schedule import plan_schedule


class _Captured(tuple):
    """The HIP graphs of a step's pieces, in order; ``rets``: what each piece returned while it was captured."""


class TrainPipeline:
    def __init__(self, model, batch, sr_in=16000, n_samp=16000, utterance_length=44, rho=0.1, constraint="product",
                 affine=None, pgd=None, dp=None, use_graph="auto", per_layer_iters=4, extractor=None, mfcc_cus="auto",
                 sync_inputs=True, overlap_buckets=False, sync_bn=False, train_cus="auto"):
        """constraint: 'product' (simple_norm_constraint, all layers), 'per_layer' (norm_constraint) or None.
        affine: (mean, scale) float64 device tensors [20*utterance_length] or None.
        pgd: dict(eps=, eps_step=, max_iter=[, norm=np.inf | 1 | 2][, num_random_init=0 | 1]) for adversarial training on the
        standardised features (norm and random start as ART's ProjectedGradientDescent).
        extractor: a feature extractor ``f(waves, mean, scale, out=)`` replacing the 2048/512 MFCC plan, e.g.
        ``speaker_recognition.WindowMfcc`` (441/220 windows -> 2020 features; pass utterance_length=101).
        mfcc_cus: how many of the GPU's CUs the feature-extraction stream may use (a CU-masked HIP stream, spread
        evenly over the XCDs); "auto" = the measured best share, None / 0 = no mask.
        train_cus: "rest" confines the classifier's stream to the CUs the extraction stream does NOT use (a second CU-masked
        stream: the chain's short kernels then never share a CU's LDS, wave slots and L1 with an MFCC workgroup), "all"
        leaves it on every CU, "auto" = "rest" with the built-in MFCC plan.
        use_graph: replay the classifier's part of a step as HIP graph(s) (True), launch its kernels one by one (False), or
        "auto": graphs for the long launch sequences (PGD adversarial training: ~440 launches per step; synchronized BatchNorm:
        one graph per segment between collectives), plain launches for the 29-kernel step -- measured at the end of round 4
        (batch 1024, MI355X): 0.411 against 0.417 ms per step over 200 steps, 0.433 against 0.444 over the driver's 20 (config 2:
        0.366 against 0.373).  The host needs 0.25 ms to enqueue a step's launches (0.09 with the graph), so it stays ahead of
        the GPU either way, and a replayed graph costs the GPU more between nodes than back-to-back launches on one queue do
        (the same graph under AMD_DIRECT_DISPATCH=0: 0.345 ms in config 2 -- but the two-stream pipeline 0.82).
        sync_inputs: order the extraction stream after the caller's current stream and the caller's stream after the
        extraction (two event hand-offs per step, ~50 us of a 0.4 ms step).  Needed whenever the tensors handed to step()
        were just produced on the caller's stream or are temporaries; a loop over a resident pool that was filled and
        synchronised beforehand (bench.py) may pass False."""
        self.sync_inputs = bool(sync_inputs)
        self._refuse_certified(model)
        if pgd:
            self._pgd_norm = _norm_value(pgd.get("norm", float("inf")))
            rinit = int(pgd.get("num_random_init", 0))
            if rinit not in (0, 1):
                raise ValueError(f"pgd num_random_init={rinit}: 0 or 1 (more restarts inside training are not supported)")
            self._pgd_rinit = rinit == 1
            self._pgd_seed = (0xBA11000000000000 + int(model._seed)) & 0xFFFFFFFFFFFFFFFF  # + the rank, folded in by the kernel
        # Data parallel, gradient exchange.  False: two HIP graphs around ONE all-reduce of the whole flat buffer.  True:
        # three graphs around two buckets, everything but [dW_0 | db_0] (44 % of the bytes) reduced beside the dW_0 GEMM.
        # Measured on one MI355X with a one-rank RCCL group (identity collectives, scratch/nccl_one_rank.py): the extra
        # graph boundary and the second collective's stream hand-offs cost +57 us per step against +14 us for the
        # one-collective schedule, more than the ~36 us of wire time the overlap can hide at this message size.
        self.overlap_buckets = bool(overlap_buckets)
        # Data parallel, BatchNorm: per-replica statistics (default; accuracy parity shown in tests/test_dp_gpu.py) or, opt-in,
        # statistics of the global batch through 2 small all-reduces per BatchNorm layer (eager launches, no HIP graph): set below
        self.model, self.batch, self.L = model, int(batch), int(utterance_length)
        self.dev = model._device
        self.h = N.get_handle(self.dev.index)
        self.ex = MfccExtractor(sr_in, n_samp, self.batch, self.dev) if extractor is None else extractor
        self._custom_ex = extractor is not None
        self.rho, self.constraint, self.pgd = float(rho), constraint, pgd
        self.dp = dp if dp is not None else DataParallel()
        model._replica_rank = self.dp.rank  # every rank draws its own dropout masks
        self._late = model.late_floats      # [dW_0 | db_0]: the gradient bucket that is ready last
        self.sync_bn = bool(sync_bn) and self.dp.world > 1
        self.per_layer_iters = per_layer_iters
        self.mean, self.scale = affine if affine is not None else (None, None)
        nf = 20 * self.L
        if model._widths[0] != nf:
            raise ValueError(f"model input width {model._widths[0]} != {nf}")
        self._nbuf = 2  # feature/label buffers in flight (a third or fourth measured no different, CU-masked or not, balanced legs or not)
        self._feats2 = [torch.zeros(self.batch, nf, device=self.dev) for _ in range(self._nbuf)]
        self._labels2 = [torch.zeros(self.batch, model._n_classes, device=self.dev) for _ in range(self._nbuf)]
        self.feats, self.labels = self._feats2[0], self._labels2[0]  # buffers of the most recent step
        self.x_adv = torch.zeros(self.batch, nf, device=self.dev) if pgd else None
        nl = len(model._blocks)
        self.norms = torch.zeros(nl + 1, device=self.dev)
        self.sigmas = torch.zeros(nl, device=self.dev)
        self.v_state = torch.zeros(sum(model._widths[1:]), device=self.dev)
        self._order = N.int_array(list(range(nl)))
        self._warm = False
        self._n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count

        def plan(cus):
            return plan_schedule(n_cu=self._n_cu, batch=self.batch, compute_dtype=getattr(model, "_compute_dtype", "float32"), pgd=bool(pgd),
                                 custom_extractor=self._custom_ex, mfcc_cus=cus, train_cus=train_cus, use_graph=use_graph, world=self.dp.world,
                                 sync_bn=self.sync_bn, constraint=constraint, has_adam_signal=N.has("lipasr_mlp_adam_project_product_signal"))

        sched = plan(mfcc_cus)  # the policy and its measurements: schedule.py
        self._masked_stream = self._masked_train_stream = None  # CU-masked streams this pipeline made (hardware queues of their own)
        self._gemm_tiles_set = False
        self.stream = torch.cuda.Stream(device=self.dev)  # training stream (equal priorities measured best)
        if sched.mfcc_groups is not None:
            self.mfcc_cus = sched.mfcc_cus  # (without a partition the attribute does not exist)
            self._masked_stream = self._make_masked_stream(0, sched.mfcc_groups, warn="the MFCC stream shares every CU")
            if self._masked_stream is None:  # a runtime without CU masking: same results, the shared-CU schedule
                sched = plan(None)
            elif hasattr(self.ex, "set"):
                # the three-kernel path's persistent resampler sizes its grid to one workgroup per CU it may use
                # (the STFT kernel's fused DCT epilogue, plan key 4, stays off: on a CU share one workgroup per clip holding its 74 kB of
                # LDS while two of its four wavefronts run the fp32 DCT loses to the separate dct_kernel -- stage 0.400 against 0.388 ms
                # on 96 CUs, step 0.434 against 0.418 ms, round 4)
                self.ex.set(1, self.mfcc_cus)
        self.use_graph = sched.use_graph
        if sched.classifier_groups is not None:
            self._masked_train_stream = self._make_masked_stream(*sched.classifier_groups)
        if self._masked_train_stream is not None:
            self.stream = torch.cuda.ExternalStream(self._masked_train_stream.value, device=self.dev)
        confined = sched.classifier == "rest" and self._masked_train_stream is not None
        self.train_cus = sched.train_cus if confined else self._n_cu  # the CUs the classifier's stream may use
        if confined:
            N.check(N.lib.lipasr_mlp_set_gemm_tiles(self.model._plan, sched.gemm_tiles))
            N.check(N.lib.lipasr_mlp_set_cu_budget(self.model._plan, sched.cu_budget))
            self._gemm_tiles_set = True  # the pipeline owns these settings: close() puts the model's plan back
        self.mfcc_stream = (torch.cuda.ExternalStream(self._masked_stream.value, device=self.dev) if self._masked_stream is not None
                            else torch.cuda.Stream(device=self.dev))  # feature-extraction stream
        # The schedule's wishes that need a stream of this pipeline's own making: an extraction that may leave its share needs a
        # share; the flags need streams that can run at the same time whatever the other one holds, i.e. a classifier stream that
        # owns a hardware queue; and the Adam kernel can only raise a flag that exists.
        self._wide_stream = torch.cuda.Stream(device=self.dev) if sched.wide and self._masked_stream is not None else None
        if sched.flags and self._masked_train_stream is not None:
            self._handoff = FlagHandoff(self.h, self._nbuf, self.dev, knobs.get("LIPASR_FLAG_TIMEOUT_MS"))
        else:
            self._handoff = EventHandoff(self._nbuf, self._wide_stream is not None)
        self._adam_signal = sched.adam_signal and self._flags is not None
        self._i = 0
        self._graphs = {}  # (bsz, b, gb) -> _Captured
        self._closed = self._failed = False
        self._prof, self._prof_i = None, 0
        N.register_owner(self)

    _flags = property(lambda self: self._handoff.flags)
    _flag_err = property(lambda self: self._handoff.err)
    _flag_timeout_ms = property(lambda self: self._handoff.timeout_ms)

    def _make_masked_stream(self, first, end, warn=None):
        """A native stream confined to the 8-CU groups first .. end - 1, or None where the runtime cannot mask (after a warning, when
        ``warn`` says what follows).  Measured on MI355X (scratch/cu_mask_probe.py): mask bits act in groups of 8 consecutive bits --
        group g (bits 8g .. 8g+7) stands for CU g of every XCD, and the group is enabled when any of its bits is set.  The
        extraction gets the first groups (an evenly spread choice measured erratic, 0.517 ... 0.78 ms, the prefix smooth), the
        classifier the others (partitions that share 32 or 64 CUs measured worse: 0.452-0.461 against 0.418 ms) or all."""
        words = (self._n_cu + 31) // 32
        mask = (C.c_uint32 * words)()
        for bit in range(8 * first, min(8 * end, self._n_cu)):
            mask[bit // 32] |= 1 << (bit % 32)
        st = N.c_s()
        if N.lib.lipasr_stream_create_masked(self.h.h, mask, words, C.byref(st)) == N.OK:
            return st
        if warn:
            import warnings

            warnings.warn(f"lipasr: CU-masked stream unavailable ({N.last_error()}); {warn}")
        return None

    def _check_flags(self):
        """Reads the pinned report word of the device-side waits (no synchronisation).  Raises once per report and clears it,
        so that close() can still drain and release the streams afterwards."""
        fe = self._handoff.err
        if fe is None:
            return
        code = int(fe[0])
        if code:
            fe[0] = 0
            self._failed = True
            what = ("is overdue (it is still waiting: nothing ran out of order)" if code == 1
                    else "gave up: what its stream did afterwards was not ordered against the other stream")
            raise RuntimeError(f"TrainPipeline: a device-side wait between the extraction and the classifier stream {what} "
                               f"after {self._flag_timeout_ms} ms without the other stream's signal; LIPASR_GPU_FLAGS=0 uses events")

    # ---- pieces (all enqueue on the current stream)
    def _pgd_loop(self, bsz, x, y):
        """PGD on x with the batch's labels into self.x_adv[:bsz].  norm inf: the fused sign-step iteration; norm 1 / 2: its Lp
        form (one launch more per iteration).  num_random_init=1: the start is x + a draw from the eps ball keyed by the model's
        device step counter and the replica rank, so every step (eager or a replayed graph) draws a fresh one."""
        m = self.model
        eps, eps_step = float(self.pgd["eps"]), float(self.pgd.get("eps_step", 0.1))
        xa = self.x_adv[:bsz]
        if self._pgd_rinit:
            N.check(N.lib.lipasr_lp_ball_init(self.h.h, N.ptr(xa), N.ptr(x), bsz, xa.shape[1], self._pgd_norm, eps, self._pgd_seed,
                                              N.ptr(m._step), self.dp.rank, N.stream_ptr()))
        else:
            xa.copy_(x)
        for _ in range(int(self.pgd.get("max_iter", 20))):
            if self._pgd_norm == float("inf"):
                N.check(N.lib.lipasr_mlp_attack_step(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xa), N.ptr(x), N.ptr(y), bsz,
                                                     eps_step, eps, N.stream_ptr()))
            else:
                N.check(N.lib.lipasr_mlp_attack_step_lp(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xa), N.ptr(x), N.ptr(y), bsz,
                                                        self._pgd_norm, eps_step, eps, N.stream_ptr()))
        return xa

    def _attack_and_train(self, bsz, b, global_batch, defer_dw0=False):
        m = self.model
        x = self._feats2[b][:bsz]
        y = self._labels2[b][:bsz]
        if self.pgd:
            x = self._pgd_loop(bsz, x, y)
        m.train_fwd_bwd(x, y, inv_batch=1.0 / float(global_batch), defer_dw0=defer_dw0)

    def _attack_only(self, bsz, b):
        """The PGD inner loop alone (inference-mode BatchNorm: nothing to synchronise); returns the training input."""
        x = self._feats2[b][:bsz]
        if not self.pgd:
            return x
        return self._pgd_loop(bsz, x, self._labels2[b][:bsz])

    def _shape(self, bsz, b, gb):
        """The classifier's part of a step, one of four shapes: its pieces (callables that enqueue on the current stream) and the
        collectives between them, in order.  ("run", piece); ("reduce", t) a blocking all-reduce and ("start", t) an asynchronous
        one of t(n), n being what the piece before returned, nothing for None; ("wait", None) for the ones started."""
        m, dp = self.model, self.dp
        if dp.world == 1:
            free = self._handoff.free_ptr(b) if self._adam_signal else None  # free[b] goes out with the Adam kernel
            return [("run", lambda: (self._attack_and_train(bsz, b, gb), self._update(free)))]
        grads, update = ("reduce", lambda n: m._grads), ("run", self._update)
        if self.sync_bn:
            # synchronized BatchNorm: [PGD loop] -> segment 0 | all-reduce | segment 1 | ... | gradient all-reduce | update
            y = self._labels2[b][:bsz]
            xin = (self.x_adv if self.pgd else self._feats2[b])[:bsz]
            sums = ("reduce", lambda n: m._part[:n] if n else None)  # the segment's BatchNorm column sums (none after the last)
            shape = [("run", lambda: (self._attack_only(bsz, b), m.syncbn_segment(0, xin, y, gb, dp.world))[1]), sums]
            for seg in range(1, m.syncbn_segments()):
                shape += [("run", lambda s=seg: m.syncbn_segment(s, xin, y, gb, dp.world)), sums]
            return shape + [grads, update]
        if self.overlap_buckets:
            # two gradient buckets (reduce what is ready while the backward pass still computes):
            # fwd/bwd without dW_0 -> [everything behind dW_0 | db_0 reduces, 44 % of the bytes] || dW_0 -> [dW_0 | db_0] -> update
            late = self._late
            return [("run", lambda: self._attack_and_train(bsz, b, gb, defer_dw0=True)), ("start", lambda n: m._grads[late:]),
                    ("run", lambda: m.train_dw0((self.x_adv if self.pgd else self._feats2[b])[:bsz])), ("start", lambda n: m._grads[:late]),
                    ("wait", None), update]
        return [("run", lambda: self._attack_and_train(bsz, b, gb)), grads, update]

    def _run_shape(self, bsz, b, gb):
        """Walks the step's shape: eager mode calls its pieces, graph mode replays them, each captured once per (bsz, b, gb) --
        the collectives (eager torch.distributed calls on the stream) sit between the same pieces in both."""
        shape = self._shape(bsz, b, gb)
        g = self._graphs.get((bsz, b, gb)) if self.use_graph else None
        if self.use_graph and g is None:
            rets = []  # (sync-BN: the segments' reduce counts; a capture runs nothing, so all pieces are captured before the first replay)
            g = _Captured(self._capture(lambda p=p: rets.append(p())) for kind, p in shape if kind == "run")
            g.rets = rets
            self._graphs[(bsz, b, gb)] = g
        k, ret, started = 0, None, []
        for kind, arg in shape:
            if kind == "run":
                if g is None:
                    ret = arg()
                else:
                    N.check(N.lib.lipasr_graph_launch(self.h.h, g[k], N.stream_ptr()))
                    ret = g.rets[k]
                k += 1
            elif kind == "wait":
                for handle in started:
                    handle.wait()
            else:
                t = arg(ret)
                if t is None:
                    continue
                if kind == "reduce":
                    self.dp.allreduce_grads(t)
                else:
                    started.append(self.dp.allreduce_async(t))

    def _update(self, free_flag=None):
        m = self.model
        if self.constraint == "product":
            # Adam + NonNeg + simple_norm_constraint in one native call (the step counter moves inside the projection)
            m.apply_adam_project_product(self.rho, self._order, self.norms, flag=free_flag, value=self._i)
            return
        m.apply_adam()
        if self.constraint == "per_layer":
            N.check(N.lib.lipasr_mlp_project_per_layer(m._plan, N.ptr(m._params), self.rho, N.ptr(self.v_state), 1, self.per_layer_iters,
                                                       N.ptr(self.sigmas), N.stream_ptr()))

    def _capture(self, fn, *args):
        gid = C.c_int()
        N.check(N.lib.lipasr_graph_begin(self.h.h, N.stream_ptr()))
        N.capture_enter()  # native destroys (finalisers the garbage collector may run now) wait until the capture is over
        try:
            fn(*args)
        finally:
            try:
                N.check(N.lib.lipasr_graph_end(self.h.h, N.stream_ptr(), C.byref(gid)))
            finally:
                N.capture_exit()
        return gid.value

    def _warm_start(self):
        if self.constraint == "per_layer" and not self._warm:
            m = self.model
            # cold power iteration once, outside any graph, so the captured step can always run warm
            N.check(N.lib.lipasr_mlp_project_per_layer(m._plan, N.ptr(m._params), self.rho, N.ptr(self.v_state), 0, 48, N.ptr(self.sigmas),
                                                       N.stream_ptr()))
            self._warm = True

    def profile_train(self, n_steps):
        """Time the classifier part (attack + fwd/bwd [+ all-reduce] + Adam + projection) of the next ``n_steps`` steps with
        HIP events recorded on the training stream around its launches; ``train_ms()`` returns the mean.  The MFCC of the
        next batch runs beside it on its own stream, so this is the classifier's time INSIDE the overlapped step."""
        self._prof = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(int(n_steps))]
        self._prof_i = 0

    def train_ms(self):
        used = self._prof[:self._prof_i]
        self._prof = None
        if not used:
            return 0.0
        used[-1][1].synchronize()
        return sum(a.elapsed_time(b) for a, b in used) / len(used)

    @staticmethod
    def _refuse_certified(model):
        """Asked when the pipeline is built and again at every step: the model may be compiled anew in between."""
        if getattr(getattr(model, "_loss", None), "certified", False):
            raise NotImplementedError("TrainPipeline does not run IBP certified training (lipasr.bounds.IBPCrossentropy): its step "
                                      "plans hold the plain step only; train with Model.fit / Model.train_on_batch")

    def step(self, waves, y_onehot, features=None, global_batch=None):
        """waves: float32 device tensor [b, n_samp] (a view into a resident pool is fine), y_onehot [b, classes].
        features: pre-extracted, already standardised [b, 20*L] features instead of waveforms (BASELINE config 2,
        the reference's own train_constraints.py flow); the MFCC stage is skipped.
        global_batch: data parallel with UNEVEN shards only (e.g. the last partial batch cut by ``shard_bounds``): the
        number of rows all ranks process in this step; default = this rank's rows x world size.
        Asynchronous: ``pipe.feats`` / ``pipe.labels`` / the model's buffers are valid after ``synchronize()``."""
        self._refuse_certified(self.model)
        bsz = (features if features is not None else waves).shape[0]
        gb = int(global_batch) if global_batch is not None else bsz * self.dp.world
        b = self._i % self._nbuf
        self._i += 1
        self.feats, self.labels = self._feats2[b], self._labels2[b]
        if self._closed:
            raise RuntimeError("TrainPipeline.step() after close()")
        self._check_flags()
        # the inputs were produced on the caller's stream (an H2D copy, a noise kernel, a slice of a pool): order the
        # extraction stream after it.  Below, the caller's stream is in turn ordered after this step's extraction, so a
        # temporary handed to step() and freed right after it is not recycled (the caching allocator re-issues a block on
        # the stream it was allocated on) while the MFCC kernels still read it.  (Not record_stream(): the allocator would
        # then record events on the CU-masked stream whenever such a block is freed -- also after close() destroyed it.)
        caller, ho, i = torch.cuda.current_stream(self.dev), self._handoff, self._i
        xs = self.mfcc_stream
        wide = self._wide_stream is not None and features is None and ho.classifier_idle(self.stream)
        if wide:  # nothing runs on the classifier's CUs: this extraction may have them
            xs = self._wide_stream
            self.ex.set(1, self._n_cu)
        if self.sync_inputs:
            xs.wait_stream(caller)
        with torch.cuda.stream(xs):
            ho.order_extraction(xs)
            ho.wait_free(b, i, xs)                    # 1. the step that last read buffer b is done with it
            if features is not None:                  # 2. the extraction
                self._feats2[b][:bsz].copy_(features)
            elif self._custom_ex:
                self.ex(waves, self.mean, self.scale, out=self._feats2[b][:bsz])
            else:
                self.ex(waves, self.L, self.mean, self.scale, out=self._feats2[b][:bsz])
            self._labels2[b][:bsz].copy_(y_onehot)
            ho.signal_ready(b, i, xs)                 # 3. features and labels of b are ready
        if wide:
            self.ex.set(1, self.mfcc_cus)
        if self.sync_inputs:
            ho.caller_waits(caller, b, xs)
        with torch.cuda.stream(self.stream):
            self._warm_start()
            ho.wait_ready(b, i, self.stream)          # 4. the classifier waits for them
            prof = None
            if self._prof is not None and self._prof_i < len(self._prof):
                prof = self._prof[self._prof_i]
                self._prof_i += 1
                prof[0].record(self.stream)
            self._run_shape(bsz, b, gb)               # 5. attack, forward / backward, collectives, update
            if prof is not None:
                prof[1].record(self.stream)
            if not self._adam_signal:                 # 6. the classifier is done with b (or its Adam kernel said so in 5)
                ho.signal_free(b, i, self.stream)

    def synchronize(self):
        if self._wide_stream is not None:
            self._wide_stream.synchronize()
        self.mfcc_stream.synchronize()
        self.stream.synchronize()
        self._check_flags()
        if self.model.exchange_errors():
            raise RuntimeError("TrainPipeline: a BatchNorm exchange inside a GEMM gave up after 2 s (workgroups of one column block were never "
                               "resident together: is the plan's CU budget larger than its stream's CU mask?); the step's results are invalid. "
                               "LIPASR_FUSE_BN=0 uses the launch chain")

    @property
    def mfcc_stream_kind(self):
        """"masked" (its own hardware queue, confined to ``mfcc_cus`` CUs) or "shared" (a pool stream on every CU)."""
        return "masked" if self._masked_stream is not None else "shared"

    def close(self):
        """Drains both streams, destroys this pipeline's graph executables and gives the CU-masked stream (a hardware
        queue of its own) back, in that order.  Idempotent; also reached from ``lipasr._native.shutdown`` at interpreter
        exit, so no HIP object of the pipeline is left to the runtime's static destructors."""
        if getattr(self, "_closed", True):
            return
        if N._capture_depth > 0:  # a finaliser in the middle of another pipeline's capture: synchronising / freeing would break it
            N._deferred.append((self.close, ()))
            return
        self._closed = True
        if not self.h.alive:  # the handle went first and took graphs and streams with it
            self._graphs.clear()
            self._masked_stream = self._masked_train_stream = None
            # the ExternalStream wrappers point at destroyed queues: nothing may synchronise on them any more
            self.stream = self.mfcc_stream = torch.cuda.current_stream(self.dev)
            return
        pending = None
        try:
            self.synchronize()
        except RuntimeError as e:  # a device-side wait reported: finish the teardown (queues, graphs), then tell the caller
            pending = e
        for g in self._graphs.values():
            for gid in g:
                N.lib.lipasr_graph_destroy(self.h.h, gid)
        self._graphs.clear()
        st = self._masked_stream
        if st is not None:
            self._masked_stream = None
            self.mfcc_stream = torch.cuda.Stream(device=self.dev)
            N.lib.lipasr_stream_destroy(self.h.h, st)
        st = self._masked_train_stream
        if st is not None:
            self._masked_train_stream = None
            self.stream = torch.cuda.Stream(device=self.dev)
            N.lib.lipasr_stream_destroy(self.h.h, st)
        if self._gemm_tiles_set and getattr(self.model, "_plan", None):
            self._gemm_tiles_set = False
            N.lib.lipasr_mlp_set_gemm_tiles(self.model._plan, 0)  # back to the library's default threshold
            N.lib.lipasr_mlp_set_cu_budget(self.model._plan, 0)
        if not self._custom_ex:
            self.ex.close()  # the pipeline's own MFCC plan
        if pending is not None:
            raise pending

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
