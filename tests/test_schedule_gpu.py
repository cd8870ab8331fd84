"""GPU: what TrainPipeline builds is what lipasr.schedule.plan_schedule says for this device, and a step issues the hand-off
protocol of lipasr/handoff.py as this order of native calls:

    wait free[b] (i - 2) -> extraction -> signal ready[b] (i) -> wait ready[b] (i) -> forward / backward -> free[b] (i)

Batch 32, the reference's constrained network, synthetic clips."""
import numpy as np
import pytest
import torch

from helpers import build_model, dev, load_params
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu

FLAG_CALLS = ("lipasr_flag_signal", "lipasr_flag_wait")
ADAM, ADAM_SIGNAL = "lipasr_mlp_adam_project_product", "lipasr_mlp_adam_project_product_signal"
FWD_BWD, LAUNCH = "lipasr_mlp_train_fwd_bwd", "lipasr_graph_launch"


@pytest.fixture(scope="module")
def clips():
    from lipasr.synth import synth_clips

    waves, labels = synth_clips(64, seed=17)
    return dev(waves), dev(P.to_categorical(labels, 10))


def _model():
    spec = P.vd_constrained_spec()
    m = build_model(spec, max_batch=32)
    load_params(m, P.init_params(spec, seed=9, dtype=np.float32, nonneg_init=True))
    return m


@pytest.mark.parametrize("kwargs", [{}, {"pgd": dict(eps=0.5, eps_step=0.1, max_iter=3)}, {"mfcc_cus": None}], ids=["defaults", "pgd", "no-partition"])
def test_pipeline_realises_the_planned_schedule(cuda, clips, kwargs):
    from lipasr import _native as N
    from lipasr.pipeline import TrainPipeline
    from lipasr.schedule import plan_schedule

    m = _model()
    n_cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    s = plan_schedule(n_cu=n_cu, batch=32, compute_dtype=m._compute_dtype, pgd=bool(kwargs.get("pgd")), mfcc_cus=kwargs.get("mfcc_cus", "auto"),
                      has_adam_signal=N.has(ADAM_SIGNAL))
    pipe = TrainPipeline(m, batch=32, rho=0.1, **kwargs)
    try:
        # this device masks streams, so the plan's wishes hold wherever the plan gives the classifier a masked stream
        assert (pipe._masked_stream is not None) == (s.mfcc_groups is not None)
        assert (pipe._masked_train_stream is not None) == (s.classifier != "pool")
        flags = s.flags and s.classifier != "pool"
        assert getattr(pipe, "mfcc_cus", None) == s.mfcc_cus and pipe.train_cus == s.train_cus
        assert pipe.mfcc_stream_kind == ("masked" if s.mfcc_groups is not None else "shared")
        assert (pipe._flags is not None) == flags and pipe._adam_signal == (s.adam_signal and flags) and pipe.use_graph == s.use_graph
        pipe.step(clips[0][:32], clips[1][:32])
        pipe.synchronize()
        assert int(m._step.item()) == 1
    finally:
        pipe.close()
        m.close()


class _Recorder:
    """lipasr._native.lib with every lipasr_* call noted by name; the flag calls (and the Adam kernel that signals) with slot and value."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lipasr_"):
            return fn

        def call(*a):
            self._log.append((name, a[1], a[2]) if name in FLAG_CALLS else (name, a[-3], a[-2]) if name == ADAM_SIGNAL else (name,))
            return fn(*a)

        return call


def _five_steps(monkeypatch, clips, env=(), use_graph=False):
    """Five steps' native calls, one list per step, and the device address of the flags (None with events)."""
    from lipasr import _native as N
    from lipasr.pipeline import TrainPipeline

    for name in ("LIPASR_GPU_FLAGS", "LIPASR_ADAM_SIGNAL", "LIPASR_TRAIN_CUS", "LIPASR_MFCC_CUS", "LIPASR_TRAIN_OWN_QUEUE"):
        monkeypatch.delenv(name, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    m = _model()
    pipe = TrainPipeline(m, batch=32, rho=0.1, constraint="product", sync_inputs=False, use_graph=use_graph)
    log, steps = [], []
    monkeypatch.setattr(N, "lib", _Recorder(N.lib, log))
    try:
        for i in range(5):
            s = (i % 2) * 32
            pipe.step(clips[0][s:s + 32], clips[1][s:s + 32])
            steps.append(list(log))
            log.clear()
        pipe.synchronize()
        assert int(m._step.item()) == 5
        base = None if pipe._flags is None else pipe._flags.data_ptr()
    finally:
        monkeypatch.undo()
        pipe.close()
        m.close()
    return steps, base


def _protocol(calls, base, i):
    """Asserts the moments 1-4 of step i (1-based) in ``calls`` and returns the positions of (ready-wait, forward / backward or None)."""
    b = (i - 1) % 2
    ready, free = base + 4 * b, base + 4 * (2 + b)
    names = [c[0] for c in calls]
    extraction = [k for k, n in enumerate(names) if n.startswith("lipasr_mfcc_") and n != "lipasr_mfcc_plan_set"]
    waits = [c for c in calls if c[0] == "lipasr_flag_wait"]
    assert extraction
    if i > 2:
        assert waits[0] == ("lipasr_flag_wait", free, i - 2) and calls.index(waits[0]) < extraction[0]
    assert len(waits) == (2 if i > 2 else 1)  # the first use of a buffer waits for nobody
    sig, wait = calls.index(("lipasr_flag_signal", ready, i)), calls.index(("lipasr_flag_wait", ready, i))
    assert extraction[-1] < sig < wait
    return wait, (names.index(FWD_BWD) if FWD_BWD in names else None)


def test_a_step_is_the_handoff_protocol_in_order(cuda, clips, monkeypatch):
    steps, base = _five_steps(monkeypatch, clips)
    for i, calls in enumerate(steps, 1):
        wait, fwd = _protocol(calls, base, i)
        free = base + 4 * (2 + (i - 1) % 2)
        assert wait < fwd < calls.index((ADAM_SIGNAL, free, i))            # "buffer free" goes out with the Adam kernel ...
        assert ("lipasr_flag_signal", free, i) not in calls and (ADAM,) not in calls  # ... and only there


def test_without_the_adam_signal_a_trailing_launch_frees_the_buffer(cuda, clips, monkeypatch):
    steps, base = _five_steps(monkeypatch, clips, env=[("LIPASR_ADAM_SIGNAL", "0")])
    for i, calls in enumerate(steps, 1):
        wait, fwd = _protocol(calls, base, i)
        adam = calls.index((ADAM,))
        assert wait < fwd < adam and calls[adam + 1] == ("lipasr_flag_signal", base + 4 * (2 + (i - 1) % 2), i)
        assert not [c for c in calls if c[0] == ADAM_SIGNAL]


def test_with_events_no_flag_entry_point_is_called(cuda, clips, monkeypatch):
    steps, base = _five_steps(monkeypatch, clips, env=[("LIPASR_GPU_FLAGS", "0")])
    assert base is None
    for calls in steps:
        names = [c[0] for c in calls]
        assert FWD_BWD in names and ADAM in names
        assert not [n for n in names if n in FLAG_CALLS or n == ADAM_SIGNAL]


def test_a_replayed_step_is_one_graph_launch_between_the_ready_wait_and_the_free_signal(cuda, clips, monkeypatch):
    steps, base = _five_steps(monkeypatch, clips, use_graph=True)
    for i, calls in enumerate(steps, 1):
        wait, fwd = _protocol(calls, base, i)
        names = [c[0] for c in calls]
        assert names.count(LAUNCH) == 1
        assert wait < names.index(LAUNCH) < calls.index(("lipasr_flag_signal", base + 4 * (2 + (i - 1) % 2), i))
        if i > 2:  # both buffers' graphs exist: nothing of the classifier is launched by hand
            assert fwd is None and ADAM not in names and "lipasr_graph_begin" not in names
