"""The hand-offs between TrainPipeline's two streams, per feature / label buffer b and step i (counted from 1):

    extraction stream:  wait free[b]  ->  extract into b  ->  signal ready[b]
    classifier stream:  wait ready[b] ->  train on b      ->  signal free[b]

as device-side counters (FlagHandoff: lipasr_flag_signal / lipasr_flag_wait, one-wavefront kernels) or as hipEventRecord +
hipStreamWaitEvent pairs (EventHandoff).  Both also order consecutive extractions -- the extraction plan's scratch is shared,
whichever of the masked and the wide stream they ran on -- and the caller's stream after an extraction that read its tensors.
Round 5: a flag wait that times out REPORTS and keeps waiting (it used to let the stream run on
onto unordered data); the report lands in a pinned host word that TrainPipeline's step(), synchronize() and close() read
without synchronising anything, so a caller that never calls pipe.synchronize() hears of it at its next step."""
import torch

from . import _native as N


class FlagHandoff:
    def __init__(self, h, nbuf, device, timeout_ms):
        self.h, self.nbuf, self.timeout_ms = h, nbuf, timeout_ms
        self.flags = torch.zeros(2 * nbuf, dtype=torch.int32, device=device)  # ready[b] | free[b]: both count steps
        self.err = torch.zeros(1, dtype=torch.int32).pin_memory()            # 1: a wait is overdue, 2: a wait gave up
        self._last_xs = None

    def free_ptr(self, b):
        return self.flags[self.nbuf + b:].data_ptr()

    def _wait(self, slot, value):
        N.check(N.lib.lipasr_flag_wait(self.h.h, self.flags[slot:].data_ptr(), value, self.timeout_ms, self.err.data_ptr(), N.stream_ptr()))

    def _signal(self, slot, value):
        N.check(N.lib.lipasr_flag_signal(self.h.h, self.flags[slot:].data_ptr(), value, N.stream_ptr()))

    def classifier_idle(self, stream):
        return stream.query()

    def order_extraction(self, xs):
        if self._last_xs is not None and self._last_xs is not xs:
            xs.wait_stream(self._last_xs)
        self._last_xs = xs

    def wait_free(self, b, i, xs):
        if i > self.nbuf:  # the buffer's first use waits for nobody
            self._wait(self.nbuf + b, i - self.nbuf)

    def signal_ready(self, b, i, xs):
        self._signal(b, i)

    def caller_waits(self, caller, b, xs):
        caller.wait_stream(xs)

    def wait_ready(self, b, i, stream):
        self._wait(b, i)

    def signal_free(self, b, i, stream):
        self._signal(self.nbuf + b, i)


class EventHandoff:
    flags = err = timeout_ms = None

    def __init__(self, nbuf, two_extraction_streams):
        self._ready = [torch.cuda.Event() for _ in range(nbuf)]
        self._free = [None] * nbuf
        self._two = two_extraction_streams
        self._last_ready = self._last_free = None

    def classifier_idle(self, stream):
        return self._last_free is None or self._last_free.query()

    def order_extraction(self, xs):
        if self._last_ready is not None and self._two:
            xs.wait_event(self._last_ready)

    def wait_free(self, b, i, xs):
        if self._free[b] is not None:
            xs.wait_event(self._free[b])

    def signal_ready(self, b, i, xs):
        self._ready[b].record(xs)
        self._last_ready = self._ready[b]

    def caller_waits(self, caller, b, xs):
        caller.wait_event(self._ready[b])

    def wait_ready(self, b, i, stream):
        stream.wait_event(self._ready[b])

    def signal_free(self, b, i, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        self._free[b] = self._last_free = ev
