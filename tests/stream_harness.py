"""The gated-stream protocol: does a C-ABI entry really do all of its work on the caller's stream?

A case names device inputs, a call f(stream), output buffers and a flag `blocks` (the entry may
synchronise the host).  run_case() first takes the expected bytes from a quiet run (the current
stream, the whole device synchronised before and after), then runs the entry on a fresh side
stream S whose queue is held back by a device-side delay:

  1. the real inputs wait in staging buffers; the buffers the entry reads hold a DECOY (another
     valid input of the same kind), the outputs the sentinel 7; the device is synchronised;
  2. on S: the delay, an event `gate`, then the copies staging -> inputs;
  3. the entry is called with S.  While `gate` has not completed, S has not run the copies yet:
     whatever the entry enqueued on any other stream runs now, reads the decoy (or scratch nobody
     has written) and the result differs from the expected bytes, deterministically.  For an entry
     that must not block the host, `gate` must still be pending AFTER the call returns (a hidden
     hipStreamSynchronize waits the delay out); for one that may block it is checked just BEFORE
     the call.  A gate that has already opened proves nothing and is a failure of its own;
  4. on S: outputs -> result buffers, then a second decoy over the inputs and the sentinel over
     the outputs.  Work the entry left running on another stream after it returned may meet these
     writes; this second check is opportunistic, NOT deterministic;
  5. S is synchronised and the results are compared with the expected bytes, bit for bit.

Every case runs twice on its stream: cold (the stream's workspace does not exist yet, pool blocks
were last freed on other streams; it may allocate, so only its results are checked) and warm
(results and the gate).  S is chosen so that the null stream runs beside it (fresh_stream), and each
gated run records an event on the null stream while S is held and waits for it: were the null stream
stuck behind S, the gate would be open afterwards and the run fails as proving nothing.

Decoys are always valid data (a rotation of the real rows: residues stay below their modulus,
doubles finite), so a stream bug shows as wrong bytes, never as a fault.  Pointer tables, plan
handles and key material are not gated; host arguments are read at call time.

The delay is torch.cuda._sleep, calibrated once with events (cycles per millisecond); if it does
not delay on the device, a chain of elementwise operations on a large tensor, calibrated the same
way, takes its place.  Per case the delay is max(FLOOR_MS, MULT x the warm host time of the call on
an idle stream), capped at MAX_DELAY_MS.
"""
import time

import numpy as np

from gpu_util import torch

SENTINEL = 7
FLOOR_MS = 20.0      # shortest delay of a warm gated run
MULT = 8.0           # ... or this many times the call's warm host time
COLD_MS = 60.0       # delay of the cold run (its gate is not asserted)
MAX_DELAY_MS = 250.0
REAL, DECOY, DECOY2 = 0, 1, 2


def words_of(a):
    """a numpy array as int64 words (zero-padded to 8 bytes)"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if b.size % 8:
        b = np.concatenate([b, np.zeros(8 - b.size % 8, dtype=np.uint8)])
    return b.view(np.int64).copy()


def rolled(a, row, k):
    """rows of `row` elements rotated by k: the same kind of data, other values"""
    a = np.ascontiguousarray(a)
    assert a.size % row == 0
    return np.roll(a.reshape(-1, row), k, axis=1).reshape(a.shape).copy()


class Case:
    """One entry's inputs, outputs and call.  Every device buffer is a tensor of int64 words."""

    def __init__(self, name, blocks=False):
        self.name, self.blocks = name, blocks
        self.ins, self.outs, self.keep = [], [], []
        self.call = None          # f(stream handle, ctx)
        self.oracle = None        # () -> list of (output index, expected numpy array)
        self.make_ctx = None      # () -> a fresh context for the side-stream runs (lazy tables)
        self.cleanup = []

    def inp(self, real, row, decoys=None, inout=False):
        """a gated input: `real` is what the entry must read; decoys default to its rows rotated"""
        t = torch()
        d1, d2 = decoys if decoys is not None else (rolled(real, row, 1), rolled(real, row, 2))
        assert not np.array_equal(real, d1) and not np.array_equal(real, d2), self.name
        staging = [t.from_numpy(words_of(x)).cuda() for x in (real, d1, d2)]
        buf = t.empty_like(staging[0])
        self.ins.append((buf, staging))
        if inout:
            self.outs.append(buf)
        return buf

    def out(self, count, itemsize=8):
        t = torch()
        buf = t.full((-(-count * itemsize // 8),), SENTINEL, dtype=t.int64, device="cuda")
        self.outs.append(buf)
        return buf

    def const(self, a):
        """device data that is not gated (keys, pointer tables, index arrays)"""
        buf = torch().from_numpy(words_of(a)).cuda()
        self.keep.append(buf)
        return buf

    def hold(self, *objs):
        self.keep.extend(objs)
        return objs[0]

    def close(self):
        torch().cuda.synchronize()
        for f in self.cleanup:
            f()
        self.cleanup = []


class StreamOrderError(AssertionError):
    pass


class Delay:
    """a device-side delay of a given length on the current torch stream"""

    def __init__(self):
        t = torch()
        self.t = t
        self.kind = "sleep"
        probe = 20_000_000
        t.cuda._sleep(1000)
        t.cuda.synchronize()
        ms = self._time(lambda: t.cuda._sleep(probe))
        self.cycles_per_ms = probe / ms if ms > 0 else float("inf")
        if ms < 1.0:  # _sleep does not delay here: a chain of elementwise passes over 256 MiB
            self.kind = "chain"
            self.big = t.ones(1 << 25, dtype=t.float64, device="cuda")
            self._pass()
            t.cuda.synchronize()
            self.ms_per_pass = self._time(lambda: [self._pass() for _ in range(8)]) / 8

    def _pass(self):
        self.big.mul_(1.0)

    def _time(self, f):
        t = self.t
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        t.cuda.synchronize()
        a.record()
        f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def enqueue(self, ms):
        assert 0 < ms <= MAX_DELAY_MS
        if self.kind == "sleep":
            self.t.cuda._sleep(int(ms * self.cycles_per_ms))
        else:
            for _ in range(max(1, int(round(ms / self.ms_per_pass)))):
                self._pass()

    def describe(self):
        if self.kind == "sleep":
            return f"torch.cuda._sleep, {self.cycles_per_ms:.0f} cycles/ms"
        return f"elementwise chain, {self.ms_per_pass:.3f} ms/pass"


_delay = None


def delay():
    global _delay
    if _delay is None:
        _delay = Delay()
    return _delay


def _pure_outs(case):
    ins = {b.data_ptr() for b, _ in case.ins}
    return [o for o in case.outs if o.data_ptr() not in ins]


def _fill(case, which):
    for o in _pure_outs(case):
        o.fill_(SENTINEL)
    for buf, staging in case.ins:
        buf.copy_(staging[which], non_blocking=True)


def quiet(case, which, ctx=None):
    """the entry on the current stream, the device synchronised before and after"""
    t = torch()
    t.cuda.synchronize()
    _fill(case, which)
    t.cuda.synchronize()
    case.call(t.cuda.current_stream().cuda_stream, ctx)
    t.cuda.synchronize()
    return [o.clone() for o in case.outs]


def _enqueue_gate(case, S, ms):
    """step 2, on S: the delay, the gate, the real inputs"""
    t = torch()
    with t.cuda.stream(S):
        delay().enqueue(ms)
        gate = t.cuda.Event()
        gate.record(S)
        for o in _pure_outs(case):  # whatever wrote an output before the gate opened is wiped
            o.fill_(SENTINEL)
        for buf, staging in case.ins:
            buf.copy_(staging[REAL], non_blocking=True)
    return gate


def _enqueue_collect(case, S, results):
    """step 4, on S: keep the outputs, then the second decoy and the sentinel"""
    t = torch()
    with t.cuda.stream(S):
        for r, o in zip(results, case.outs):
            r.copy_(o, non_blocking=True)
        for o in _pure_outs(case):
            o.fill_(SENTINEL)
        for buf, staging in case.ins:
            buf.copy_(staging[DECOY2], non_blocking=True)


def fresh_stream(tries=8):
    """a fresh torch stream on which a delay does not hold the null stream back.  HIP deals its streams
    round robin onto a few hardware queues (4 by default), the null stream's among them: a side stream
    that shares the null stream's queue serialises with it, and work wrongly issued on stream 0 would
    wait for the gate like the rest.  Such a stream is passed over (a 1 ms delay shows it)."""
    t = torch()
    for _ in range(tries):
        S = t.cuda.Stream()
        t.cuda.synchronize()
        with t.cuda.stream(S):
            delay().enqueue(1.0)
            gate = t.cuda.Event()
            gate.record(S)
        probe = t.cuda.Event()
        probe.record(t.cuda.default_stream())
        probe.synchronize()
        independent = not gate.query()
        S.synchronize()
        if independent:
            return S
    raise StreamOrderError(f"none of {tries} fresh side streams runs beside stream 0: nothing can be shown here")


def gated(case, S, ms, ctx=None, check_gate=True):
    """steps 1-5 once; returns (results, host seconds of the call)"""
    t = torch()
    t.cuda.synchronize()
    _fill(case, DECOY)
    results = [t.empty_like(o) for o in case.outs]
    t.cuda.synchronize()
    gate = _enqueue_gate(case, S, ms)
    probe = t.cuda.Event()
    probe.record(t.cuda.default_stream())
    probe.synchronize()  # the null stream is not held behind S
    held_before = not gate.query()
    t0 = time.perf_counter()
    case.call(S.cuda_stream, ctx)
    host = time.perf_counter() - t0
    held_after = not gate.query()
    _enqueue_collect(case, S, results)
    S.synchronize()
    t.cuda.synchronize()
    if check_gate:
        if not held_before:
            raise StreamOrderError(f"{case.name}: the gate of {ms:.0f} ms opened before the call: the case proves nothing")
        if not case.blocks and not held_after:
            raise StreamOrderError(f"{case.name}: the gate of {ms:.0f} ms opened during a call of {host * 1e3:.2f} ms "
                                   "host time: the entry waited for the stream (documented as not synchronising), "
                                   "or the delay is too short")
    return results, host


def differ(got, want):
    """indices of the outputs whose bytes differ"""
    t = torch()
    return [i for i, (g, w) in enumerate(zip(got, want)) if not t.equal(g, w)]


def warm_delay_ms(host_seconds):
    return min(MAX_DELAY_MS, max(FLOOR_MS, MULT * host_seconds * 1e3))


def run_case(case, log=None):
    """the whole protocol for one case; raises StreamOrderError with a message of its own for each
    way to fail"""
    t = torch()
    try:
        want = quiet(case, REAL)
        if case.ins and not differ(quiet(case, DECOY), want):
            raise StreamOrderError(f"{case.name}: the decoy gives the same bytes as the real input")
        if case.oracle is not None:
            for i, exp in case.oracle():
                got = want[i].cpu().numpy()[:words_of(exp).size]
                if not np.array_equal(got, words_of(exp)):
                    raise StreamOrderError(f"{case.name}: quiet run differs from the oracle at output {i}")
        ctx = case.make_ctx() if case.make_ctx else None
        S = fresh_stream()
        cold, _ = gated(case, S, COLD_MS, ctx, check_gate=False)
        bad = differ(cold, want)
        if bad:
            raise StreamOrderError(f"{case.name}: cold call on a held side stream: outputs {bad} differ from the "
                                   "quiet run (work on another stream, or a table not ordered before its reader)")
        t.cuda.synchronize()
        _fill(case, REAL)
        t.cuda.synchronize()
        t0 = time.perf_counter()
        case.call(S.cuda_stream, ctx)
        host = time.perf_counter() - t0
        t.cuda.synchronize()
        ms = warm_delay_ms(host)
        warm, host2 = gated(case, S, ms, ctx, check_gate=True)
        bad = differ(warm, want)
        if bad:
            raise StreamOrderError(f"{case.name}: warm call on a held side stream: outputs {bad} differ from the "
                                   "quiet run")
        if log is not None:
            log(f"{case.name}: idle host {host * 1e3:.3f} ms, delay {ms:.0f} ms, gated host {host2 * 1e3:.3f} ms")
    finally:
        case.close()


def run_pair(a, b, rounds=4, ms=40.0):
    """two instances on one context, each on its own held stream, calls issued alternately so both
    queues are full when the gates open; every round's result must equal that instance's quiet
    bytes.  Catches scratch or tables shared across streams when the kernels overlap: NOT
    deterministic."""
    t = torch()
    try:
        cases = (a, b)
        want = [quiet(c, REAL) for c in cases]
        streams = [fresh_stream(), fresh_stream()]
        for c, S in zip(cases, streams):  # warm each stream's workspace
            _fill(c, REAL)
            t.cuda.synchronize()
            c.call(S.cuda_stream, None)
        t.cuda.synchronize()
        for c in cases:
            _fill(c, DECOY)
        results = [[[t.empty_like(o) for o in c.outs] for _ in range(rounds)] for c in cases]
        t.cuda.synchronize()
        gates = [_enqueue_gate(c, S, ms) for c, S in zip(cases, streams)]
        for r in range(rounds):
            for k, (c, S) in enumerate(zip(cases, streams)):
                if r:
                    with t.cuda.stream(S):
                        for buf, staging in c.ins:
                            buf.copy_(staging[REAL], non_blocking=True)
                c.call(S.cuda_stream, None)
                _enqueue_collect(c, S, results[k][r])
        held = [not g.query() for g in gates]
        for S in streams:
            S.synchronize()
        t.cuda.synchronize()
        if not all(held) and not (a.blocks or b.blocks):
            raise StreamOrderError(f"{a.name}: a gate of {ms:.0f} ms opened before all {2 * rounds} calls were issued")
        for k, c in enumerate(cases):
            for r in range(rounds):
                bad = differ(results[k][r], want[k])
                if bad:
                    raise StreamOrderError(f"{c.name}: instance {k}, round {r}: outputs {bad} differ from the quiet run")
    finally:
        a.close()
        b.close()
