"""Helpers of tests/test_gpu_stream_order.py: which entry points of include/srcfd.h take a stream, a calibrated delay
kernel, and the one routine every test there goes through -- `delayed_call`: the inputs of a call reach their final
addresses BEHIND a delay on a non-blocking side stream, the call under test is enqueued behind them on the same stream,
and its outputs are cloned on that stream.  A launch that left the stream, or an internal stream that is not fenced
against it, then reads the decoys that sat at those addresses before (valid data, other numbers); work that is not joined
back into the stream is missing from the clones.
"""
import os
import re
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "srcfd.h")

# The delay in front of every delayed arrival.  It has to outlast the host-side enqueue of the call under test (condition
# "the stream was still busy when the call returned"); the longest enqueue is a training step that captures and instantiates
# its graph (a few milliseconds).  Lengthen it if that condition ever fails on a slower host.
DELAY_MS = 100.0


def stream_entry_points(header_text=None):
    """Names of the functions of include/srcfd.h that have a `hip_stream` parameter."""
    if header_text is None:
        with open(HEADER) as f:
            header_text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = set()
    for m in re.finditer(r"\b(srcfd_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"\bhip_stream\b", m.group(2)):
            names.add(m.group(1))
    return names


class Delay:
    """`enqueue(stream)`: the stream is busy for about DELAY_MS from the moment it gets there.  One spinning thread
    (torch.cuda._sleep) whose clock is calibrated once against HIP events; a chain of matrix products of the same measured
    length where that kernel is not available."""

    def __init__(self, torch, ms=DELAY_MS):
        self.torch = torch
        self.ms = ms
        self.stream = torch.cuda.Stream()
        self.cycles = None
        self.matmuls = None
        try:
            cycles = 2_000_000
            t = self._time(lambda: torch.cuda._sleep(cycles))
            if t < 1.0:                      # a fast clock: measure a stretch long enough for the events' resolution
                cycles *= 50
                t = self._time(lambda: torch.cuda._sleep(cycles))
            self.cycles = max(1, int(cycles * ms / t))
        except (RuntimeError, AttributeError):
            self.a = torch.randn((2048, 2048), device="cuda")
            self.b = torch.empty_like(self.a)
            self._chain(4)                   # library set-up outside the timed stretch
            t = self._time(lambda: self._chain(16))
            self.matmuls = max(1, int(16 * ms / t) + 1)
        self.measured_ms = self._time(lambda: self._spin())

    def _chain(self, k):
        for _ in range(k):
            self.torch.mm(self.a, self.a, out=self.b)

    def _time(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record()
            fn()
            e1.record()
        self.stream.synchronize()
        return max(float(e0.elapsed_time(e1)), 1e-3)

    def _spin(self):
        if self.cycles is not None:
            self.torch.cuda._sleep(self.cycles)
        else:
            self._chain(self.matmuls)

    def enqueue(self, stream):
        with self.torch.cuda.stream(stream):
            self._spin()


class Arrival:
    """One input buffer of a call: `dst` holds `decoy` before anything is enqueued; `real` is copied over it behind the
    delay.  All three are device tensors of one shape and dtype, `decoy` and `real` finite-valued and different."""

    def __init__(self, dst, decoy, real):
        assert dst.shape == decoy.shape == real.shape and dst.dtype == decoy.dtype == real.dtype
        self.dst, self.decoy, self.real = dst, decoy, real


class Outcome:
    def __init__(self, clones, pending, enqueue_s):
        self.clones = clones          # the outputs as the side stream saw them after the call
        self.pending = pending        # the stream was still busy when the call under test returned
        self.enqueue_s = enqueue_s    # host time of the call under test


# the slowest enqueue of a call under test seen in this process, (seconds, label): printed by the tests, for the record
longest_enqueue = [0.0, ""]


def delayed_call(torch, delay, stream, arrivals, call, outputs, stale=(), label=""):
    """Decoys in place -> [on `stream`: delay, the real inputs, `call()`, clones of `outputs`] -> synchronise `stream`.
    stale: (tensor, contents) pairs written before anything is enqueued, so that the outputs start from known, valid, WRONG
    contents.  `call` must enqueue on `stream` (it is made with `stream` as torch's current stream)."""
    for a in arrivals:
        a.dst.copy_(a.decoy)
    for t, contents in stale:
        t.copy_(contents)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delay.enqueue(stream)
        for a in arrivals:
            a.dst.copy_(a.real, non_blocking=True)
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        pending = not stream.query()
        clones = [o.clone() for o in outputs]
    stream.synchronize()
    if dt > longest_enqueue[0]:
        longest_enqueue[:] = [dt, label]
    return Outcome(clones, pending, dt)


def assert_pending(outcome, what):
    assert outcome.pending, (f"{what}: the side stream had drained when the call returned -- either the call synchronised (the header "
                             f"promises it does not) or the {DELAY_MS:g} ms delay did not outlast its {outcome.enqueue_s * 1e3:.1f} ms enqueue; "
                             "the delayed-arrival check proves nothing in that state")


def bits(t):
    """Integer view of a tensor for bit-for-bit comparison (NaN-safe, -0 != +0)."""
    torch = __import__("torch")
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}.get(t.dtype)
    return t.view(view) if view is not None else t


def assert_bit_equal(got, want, what):
    torch = __import__("torch")
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not torch.equal(bits(got), bits(want)):
        diff = bits(got) != bits(want)
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ from the default-stream result "
                             f"(first at flat index {int(diff.flatten().nonzero()[0])})")
