"""Two conditions of the calling contract that every header states, for every wrapper family (tests/contract_cases.py):

  "all device work goes to the caller's stream"   -- the case runs on a side stream whose inputs arrive late: the device
      tensors hold a DECOY (a valid input of the same shapes), and the copies of the real inputs over it are enqueued on
      the side stream behind a delay (``torch.cuda._sleep``). ``_lib.call`` is patched to enqueue the same delay in front of
      every entry point and to assert that the stream it passes is the side stream's. A launch, memset or copy that goes to
      stream 0 or to a private stream, or a read-back that waits on the wrong stream, then sees the decoy, an earlier
      kernel's missing output or an unwritten error word: the outputs differ from the baseline's bytes, or a refusal that
      is detected on the device does not raise.
  "nothing is assumed about the workspace's contents" -- ``_lib.workspace`` is patched to hand out the same buffers call
      after call (one per position in a run, allocated once at the largest size any run asks for and sliced), so the real
      case runs on what a decoy of the same size, and one of twice the size, left behind: in the workspaces and in the
      library's own per-device scratch. The leftovers of a valid run are in range, as in production; no byte patterns.

What the side-stream part does NOT detect: a misdirected launch that is the FIRST one after an internal host
synchronisation of the entry point (the delay in front of the call has drained by then, and the inputs are in place). That
gap is covered by reading: every launch, memset and copy in csrc/ names its stream, and the entry points without a stream
parameter promise in their headers what they do (include/otto_covis.h, include/otto_mf.h).

``test_the_method_is_sensitive`` shows with torch ops alone that the arrangement orders work as assumed: the consuming
op on the default stream gives the decoy's result, on the side stream the real one. The side stream is chosen by that
probe (``side_stream``): streams that share a hardware queue with the default stream run in order with it whatever their
flags, and on such a stream misdirected work would be ordered by accident."""
import time

import numpy as np
import pytest

import contract_cases as cc

pytestmark = pytest.mark.gpu

FLOOR_MS = 20.0          # the delay is at least this ...
HOST_FACTOR = 10.0       # ... and at least this many times the host wall time of the case's run in the baseline
MARGIN = 1.3             # cycles are asked for this much above the bound (the cycle rate is measured, not known)

# families whose outputs are not bit-reproducible run to run: name -> reason. Their later comparisons use check().
NOT_REPRODUCIBLE = {
    'mf-train': 'the single-GPU SparseAdam step and the BPR batch step add the gradients of duplicate rows with float atomics, in the '
                'order the waves arrive (csrc/otto_mf.hip, k_rmf_acc and k_bpr_acc); the family compares them within 1e-4',
}


@pytest.fixture(scope='module')
def lib(gpu_device):
    import __graft_entry__ as g
    g.build()
    from otto_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope='module')
def clock(gpu_device):
    """Cycles of ``torch.cuda._sleep`` per millisecond on this device, measured once with two events."""
    import torch
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize(gpu_device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20_000_000
    e0.record()
    torch.cuda._sleep(n)
    e1.record()
    torch.cuda.synchronize(gpu_device)
    per_ms = n / e0.elapsed_time(e1)
    print(f'contract: torch.cuda._sleep runs {per_ms:.0f} cycles per ms')
    assert per_ms > 0
    return per_ms


def late_copy_probe(dev, side, cycles, on_side):
    """torch ops only. A tensor holds a decoy; on ``side``: a delay, then the copy of the real values over it. The consuming
    op is issued on ``side`` or on the default stream. Returns (the op saw the real values, the delay in ms)."""
    import torch
    real = torch.arange(1 << 16, dtype=torch.int64, device=dev)
    decoy = real + 1_000_000
    x = decoy.clone()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        x.copy_(real, non_blocking=True)
        if on_side:
            y = x * 2
    if not on_side:
        y = x * 2                                             # the default stream: not ordered behind the side stream
    side.synchronize()
    torch.cuda.synchronize(dev)
    saw_real = torch.equal(y, real * 2)
    assert saw_real or torch.equal(y, decoy * 2)
    assert torch.equal(x, real)
    return saw_real, e0.elapsed_time(e1)


SIDE_STREAMS_TRIED = 8


@pytest.fixture(scope='module')
def side_stream(gpu_device, clock):
    """A side stream whose work the default stream does NOT wait for. The runtime maps streams onto a few hardware queues,
    and two streams that share one run in order whatever their flags; on such a stream work misdirected to stream 0 would be
    ordered by accident and the test would see nothing. So the first of a few streams that the probe shows to run beside
    the default stream is taken; ``test_the_method_is_sensitive`` fails when there is none."""
    import torch
    cycles = int(FLOOR_MS * MARGIN * clock)
    tried = []
    for _ in range(SIDE_STREAMS_TRIED):
        side = torch.cuda.Stream(device=gpu_device)
        saw_real, ms = late_copy_probe(gpu_device, side, cycles, on_side=False)
        tried.append((side.cuda_stream, saw_real, round(ms, 1)))
        if not saw_real:
            print(f'contract: side stream {len(tried)} of {SIDE_STREAMS_TRIED} runs beside the default stream (delay {ms:.1f} ms)')
            return side
    print(f'contract: no side stream runs beside the default stream: {tried}')
    return None


@pytest.fixture(autouse=True)
def stop_after_a_device_fault(gpu_device):
    """A device fault is sticky: every later call fails too. End the session at the first one instead of launching the
    remaining cases on a device that has faulted."""
    import torch
    yield
    try:
        torch.cuda.synchronize(gpu_device)
    except RuntimeError as e:
        pytest.exit(f'the device reports an error after this test, no further case is run: {e}', returncode=3)


class Reused:
    """``_lib.workspace`` that keeps its buffers: the i-th request of a run gets the i-th buffer, sliced. The buffers are
    allocated once, at the largest size the sizing runs (real, decoy, double-size decoy) asked for at that position; a
    request they did not foresee would get fresh memory, that is no reused scratch, so it is an error."""

    def __init__(self, sizes, dev):
        import torch
        self.bufs = [torch.empty(n, dtype=torch.uint8, device=dev) for n in sizes]
        self.i = 0

    def begin(self):
        self.i = 0

    def __call__(self, n_bytes, dev):
        n = max(int(n_bytes), 256)
        i, self.i = self.i, self.i + 1
        assert i < len(self.bufs), f'workspace request {i} of a run: the sizing runs made {len(self.bufs)}'
        assert self.bufs[i].numel() >= n, f'workspace request {i}: {n} bytes, the sizing runs asked for {self.bufs[i].numel()} at most'
        assert self.bufs[i].device == dev
        return self.bufs[i][:n]


class State:
    """What the parts of one case share: inputs, the baseline's outputs and host time, the kept workspaces."""

    def __init__(self, case, lib, dev):
        import torch
        self.case, self.lib, self.dev = case, lib, dev
        self.real, self.decoy, self.decoy2 = case.make(cc.REAL_SEED), case.make(cc.DECOY_SEED), case.make(cc.DECOY_SEED, 2)
        sizes, self.reached = [], set()
        orig_ws, orig_call = lib.workspace, lib.call

        def ws(n_bytes, d):
            sizes.append(max(int(n_bytes), 256))
            return orig_ws(n_bytes, d)

        def call(name, d, *args, **kw):
            self.reached.add(name)
            return orig_call(name, d, *args, **kw)

        mp = pytest.MonkeyPatch()
        try:
            mp.setattr(lib, 'workspace', ws)
            mp.setattr(lib, 'call', call)
            self.baseline = self.run(self.real)
            self.reached_by_real = set(self.reached)
            first = list(sizes)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            self.second = self.run(self.real)
            torch.cuda.synchronize(dev)
            self.host_ms = (time.perf_counter() - t0) * 1e3
            both = first
            for inputs in (self.decoy, self.decoy2):           # sizes the kept buffers: the largest any run asks for
                del sizes[:]
                self.run(inputs)
                both = [max(a, b) for a, b in zip(both, sizes)] + both[len(sizes):] + sizes[len(both):]
        finally:
            mp.undo()
        self.reused = Reused(both, dev)

    def run(self, inputs, ctx=None):
        d = cc.upload(self.dev, inputs, self.case.host_keys)
        return self.outputs(self.case.run(self.dev, d, ctx) if self.case.context else self.case.run(self.dev, d))

    def outputs(self, out):
        import torch
        torch.cuda.synchronize(self.dev)
        return [cc.host(o).copy() for o in out]

    def run_reused(self, mp, inputs, ctx=None):
        self.reused.begin()
        mp.setattr(self.lib, 'workspace', self.reused)
        return self.run(inputs, ctx)

    def assert_same(self, got, what):
        if self.case.name in NOT_REPRODUCIBLE:
            self.case.check(self.real, got)
            return
        assert len(got) == len(self.baseline), what
        for i, (g, b) in enumerate(zip(got, self.baseline)):
            assert cc.same_bytes(g, b), f'{self.case.name}: output {i} {what} differs from the baseline'


_states = {}


def _fixture(cases):
    def state(request, lib, gpu_device):
        case = request.param
        if case.name not in _states:
            _states[case.name] = State(case, lib, gpu_device)
        return _states[case.name]
    return pytest.fixture(params=cases, ids=lambda c: c.name)(state)


state = _fixture(cc.CASES)
context_state = _fixture([c for c in cc.CASES if c.context])
refusal_state = _fixture([c for c in cc.CASES if c.refusals])


# ---- 0. baseline ---------------------------------------------------------------------------------------------------------------
def test_baseline_passes_the_family_check_and_repeats(state):
    state.case.check(state.real, state.baseline)
    state.assert_same(state.second, 'of a second run')
    missing = set(state.case.entry_points) - state.reached_by_real
    assert not missing, f'{state.case.name} does not reach {sorted(missing)}'


# ---- 1. reused scratch ---------------------------------------------------------------------------------------------------------
def test_reused_scratch_after_a_decoy_of_the_same_size(state, monkeypatch):
    state.run_reused(monkeypatch, state.decoy)
    state.assert_same(state.run_reused(monkeypatch, state.real), 'on the scratch of a same-size decoy')


def test_reused_scratch_after_a_decoy_of_twice_the_size(state, monkeypatch):
    state.run_reused(monkeypatch, state.decoy2)
    state.assert_same(state.run_reused(monkeypatch, state.real), 'on the scratch of a double-size decoy')


def test_context_reused_after_reset(context_state, monkeypatch):
    state, case = context_state, context_state.case
    ctx = case.new_context(state.dev, state.real)
    state.run_reused(monkeypatch, state.decoy, ctx)
    case.reset(ctx)
    state.assert_same(state.run_reused(monkeypatch, state.real, ctx), 'on a context that ran the decoy and was reset')


# ---- 2. side stream with late inputs ---------------------------------------------------------------------------------------------
class SideStream:
    """The late-input arrangement: a side stream held by a delay, ``_lib.call`` delaying every entry point on it."""

    def __init__(self, state, mp, clock, side):
        import torch
        assert side is not None, 'no side stream runs beside the default stream: this arrangement shows nothing here'
        self.state, self.torch = state, torch
        self.side = side
        self.bound_ms = max(FLOOR_MS, HOST_FACTOR * state.host_ms)
        self.cycles = int(self.bound_ms * MARGIN * clock)
        self.calls = []
        lib, orig = state.lib, state.lib.call

        def call(name, dev, *args, stream=True):
            if dev is not None and stream:
                current = torch.cuda.current_stream(dev).cuda_stream
                assert current == self.side.cuda_stream and current != 0, f'{name} is not called on the side stream'
                torch.cuda._sleep(self.cycles)
                self.calls.append(name)
            return orig(name, dev, *args, stream=stream)

        spy = lib._stream_of

        def stream_of(dev):
            s = spy(dev)
            assert s.value == self.side.cuda_stream and s.value, 'the stream passed to the library is not the side stream'
            return s

        mp.setattr(lib, 'call', call)
        mp.setattr(lib, '_stream_of', stream_of)

    def late(self, first, then):
        """Device inputs holding ``first``; on the side stream: the delay, then the copies of ``then`` over them. Returns
        the device inputs and the two events around the delay."""
        torch, st = self.torch, self.state
        d = cc.upload(st.dev, first, st.case.host_keys)
        src = cc.upload(st.dev, then, st.case.host_keys)
        torch.cuda.synchronize(st.dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.side)
        torch.cuda._sleep(self.cycles)
        e1.record(self.side)
        for k, v in src.items():
            if hasattr(v, 'copy_') and hasattr(d[k], 'copy_'):
                d[k].copy_(v, non_blocking=True)
            else:
                d[k] = v                                      # host data: the wrapper uploads it on the current stream
        return d, (e0, e1)

    def check_delay(self, events):
        ms = events[0].elapsed_time(events[1])
        print(f'contract: {self.state.case.name}: host {self.state.host_ms:.2f} ms, bound {self.bound_ms:.1f} ms, measured delay {ms:.1f} ms'
              f' in front of {len(self.calls)} entry point calls')
        assert ms >= self.bound_ms, f'the delay of {ms:.1f} ms is below max({FLOOR_MS} ms, {HOST_FACTOR} x host {self.state.host_ms:.2f} ms)'


def test_side_stream_with_late_inputs(state, monkeypatch, clock, side_stream):
    import torch
    case = state.case
    ctx = case.new_context(state.dev, state.real) if case.context else None
    state.run_reused(monkeypatch, state.decoy, ctx)            # the workspace as the decoy run left it
    if ctx is not None:
        case.reset(ctx)
    state.reused.begin()
    side = SideStream(state, monkeypatch, clock, side_stream)
    with torch.cuda.stream(side.side):
        d, events = side.late(state.decoy, state.real)
        out = case.run(state.dev, d, ctx) if case.context else case.run(state.dev, d)
    side.side.synchronize()
    side.check_delay(events)
    assert set(case.entry_points) <= set(side.calls)
    state.assert_same(state.outputs(out), 'on a side stream behind late inputs')


def test_side_stream_refusals_still_raise(refusal_state, monkeypatch, clock, side_stream):
    import torch
    state, case = refusal_state, refusal_state.case
    side = SideStream(state, monkeypatch, clock, side_stream)
    for name, (edit, call, match) in case.refusals.items():
        bad = edit(state.real) if edit is not None else state.real
        assert all(np.shape(bad[k]) == np.shape(state.real[k]) for k in bad), name
        with torch.cuda.stream(side.side):
            d, events = side.late(state.decoy, bad)
            with pytest.raises(state.lib.OttoError, match=match):
                call(state.dev, d)
        side.side.synchronize()
        side.check_delay(events)
    # the library is still usable afterwards, and the error words are clean
    monkeypatch.undo()
    state.assert_same(state.run(state.real), 'after the refusals')


# ---- 3. the method is sensitive ----------------------------------------------------------------------------------------------------
def test_the_method_is_sensitive(gpu_device, clock, side_stream):
    """torch ops only: behind the delay the late copy has not landed when an op on the default stream reads the tensor (it
    gives the decoy's result), while the same op on the side stream is ordered behind the copy (the real result)."""
    assert side_stream is not None, f'the default stream waited for each of {SIDE_STREAMS_TRIED} side streams'
    cycles = int(FLOOR_MS * MARGIN * clock)
    assert side_stream.cuda_stream != 0
    saw_real, ms = late_copy_probe(gpu_device, side_stream, cycles, on_side=False)
    assert ms >= FLOOR_MS and not saw_real, 'issued on the default stream, the op must give the decoy\'s result'
    saw_real, ms = late_copy_probe(gpu_device, side_stream, cycles, on_side=True)
    assert ms >= FLOOR_MS and saw_real, 'issued on the side stream, the op must give the real result'
