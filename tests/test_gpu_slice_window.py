"""GPU: the batched slice with its runs dispatched window by window (slice_order.h) == the
oracle's deltas, bit-exact: slice bytes plus status, has_delta, offset_from_epoch, len and
out_off per request.

Engines with 64- and 256-byte segments, so a few KB of log span many windows; the window W is
forced to 1, 2 and 5 segments with CLONOS_GATHER_WINDOW, and left at its default (2 MiB of
log: one window at these segment sizes, so the runs are only grouped by log).  One scene
serves every case: log A with eight consumers -- at 0, on a window boundary of every forced W
(10 segments) and one byte either side of it, two at equal offsets, on another boundary of
W = 1 and 2 (64 segments) and a byte past it, and at the log's end (empty delta) -- log B
with two consumers inside one segment, log C with one consumer a byte before a boundary; the
requests of the three logs interleaved.  A consumer gets to its offset as it would in use: it
took a delta when the log was that long.  The oracle's answers are computed once per segment
size.  A second scene with 16 KiB segments has logs longer than the default window, with
consumers on its boundary, either side of it, and before it.
"""
import ctypes

import numpy as np
import pytest

import _oracle as O
from clonos_amd import CausalLogID, Engine
from clonos_amd import _lib

pytestmark = pytest.mark.gpu

WINDOWS = [1, 2, 5, None]  # None: the default
BIG_SEG = 16384


def scene(seg):
    """(log lengths, requests): a request is (log, channel, the consumer's offset)."""
    if seg == BIG_SEG:  # the default window (2 MiB of log) cuts it: consumers on that boundary and around it
        w = 2 << 20
        lens = [w + 3 * seg + 11, w + seg]
        reqs = [(0, (c + 1, 0), o) for c, o in enumerate([w - 1, 0, w, w + 1, w - 3 * seg + 7, w])]
        reqs += [(1, (1, 1), w - 2), (1, (2, 1), w + seg)]
        return lens, [reqs[j] for j in (0, 6, 1, 2, 7, 3, 4, 5)]
    lens = [70 * seg + 13, 66 * seg, 65 * seg + 7]
    a = [0, 10 * seg - 1, 10 * seg, 10 * seg + 1, 10 * seg + 1, 64 * seg, 64 * seg + 1, lens[0]]
    reqs = [(0, (c + 1, 0), o) for c, o in enumerate(a)]
    reqs += [(1, (1, 1), 3 * seg + 5), (1, (2, 1), 3 * seg + 9), (2, (1, 2), 64 * seg - 1)]
    order = np.random.default_rng(seg).permutation(len(reqs))
    return lens, [reqs[j] for j in order]


def log_bytes(seg, lens):
    rng = np.random.default_rng(1000 + seg)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]


def stage(logs, seg, take):
    """Appends each log's bytes, stopping at every consumer offset above 0 for those consumers
    to take a delta there (take(log index, channel)): after it every log is whole and every
    consumer stands at its offset."""
    lens, reqs = scene(seg)
    data = log_bytes(seg, lens)
    for i, log in enumerate(logs):
        at = 0
        for stop in sorted({o for l, _, o in reqs if l == i and o > 0} | {lens[i]}):
            log_append(log, data[i][at:stop])
            at = stop
            for l, ch, o in reqs:
                if l == i and o == stop:
                    take(i, ch)
    return lens, reqs


def log_append(log, b):
    if isinstance(log, O.OracleLog):
        assert log.append(0, b) == 0
    else:
        log.appendDeterminant(b, 0)


_expected = {}


def expected(seg):
    """The oracle's answer to every request of the scene: (has_delta, offset_from_epoch, bytes)."""
    if seg not in _expected:
        refs = [O.OracleLog(seg) for _ in scene(seg)[0]]

        def take(i, ch):
            assert refs[i].has_delta(ch, 0) == (0, True)
            assert refs[i].get_delta(ch, 0)[0] == 0
        lens, reqs = stage(refs, seg, take)
        want = []
        for i, ch, o in reqs:
            st, has = refs[i].has_delta(ch, 0)
            assert st == 0
            if has:
                off = refs[i].offset(ch)[1]
                st, d = refs[i].get_delta(ch, 0)
                assert st == 0 and len(d) == lens[i] - o
                want.append((True, off, d))
            else:
                want.append((False, 0, b""))
        assert sum(1 for h, _, d in want if not d) == 1  # the consumer at the log's end
        _expected[seg] = want
    return _expected[seg]


def open_engine(monkeypatch, seg, w, **kw):
    """The switch is read when the engine is created."""
    if w is None:
        monkeypatch.delenv("CLONOS_GATHER_WINDOW", raising=False)
    else:
        monkeypatch.setenv("CLONOS_GATHER_WINDOW", str(w))
    return Engine(segment_bytes=seg, pool_segments=4096, **kw)


def staged_engine_logs(eng, seg):
    logs = [eng.open_log(CausalLogID.main(v)) for v in range(len(scene(seg)[0]))]

    def take(i, ch):
        assert logs[i].hasDeltaForConsumer(ch, 0)
        logs[i].getDeltaForConsumer(ch, 0)
    _, reqs = stage(logs, seg, take)
    return logs, reqs


def check_results(res, data, want, failed=()):
    """res rows against the oracle; out_off is the packed place in request order (a failed or
    empty request takes no room)."""
    dst = 0
    for k, ((st, has, off, n, oo), (h2, off2, d2)) in enumerate(zip(res, want)):
        if k in failed:
            assert st == _lib.CLG_E_CAPACITY and n == 0
            continue
        assert st == 0 and has == h2, k
        assert oo == dst, k
        if has:
            assert off == off2 and n == len(d2), k
            assert bytes(data[oo:oo + n]) == d2, k
        else:
            assert n == 0, k
        dst += n
    return dst


class DeviceBuf:
    """Device memory from the engine's own HIP runtime (not torch's bundled one)."""

    def __init__(self, n):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.p = ctypes.c_void_p()
        self.n = n
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(n)) == 0

    def host(self):
        h = np.empty(self.n, np.uint8)
        assert self.hip.hipMemcpy(ctypes.c_void_p(h.ctypes.data), self.p, ctypes.c_size_t(self.n), 2) == 0
        return h

    def free(self):
        self.hip.hipFree(self.p)


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("seg", [64, 256])
def test_host_output(monkeypatch, seg, w):
    want = expected(seg)
    with open_engine(monkeypatch, seg, w) as eng:
        logs, reqs = staged_engine_logs(eng, seg)
        res, out, total = eng.slice_batch([(logs[i], ch, 0) for i, ch, _ in reqs])
        assert check_results(res, out, want) == total == sum(len(d) for _, _, d in want)
        # every consumer now stands at its log's end
        res, _, total = eng.slice_batch([(logs[i], ch, 0) for i, ch, _ in reqs])
        assert total == 0 and all(st == 0 and not has and n == 0 for st, has, _, n, _ in res)


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("seg", [64, 256])
def test_device_output(monkeypatch, seg, w):
    want = expected(seg)
    need = sum(len(d) for _, _, d in want)
    buf = DeviceBuf(need + 64)
    try:
        with open_engine(monkeypatch, seg, w) as eng:
            logs, reqs = staged_engine_logs(eng, seg)
            res, _, total = eng.slice_batch([(logs[i], ch, 0) for i, ch, _ in reqs], out=buf.p.value, cap=need)
            eng.sync()
            assert check_results(res, buf.host(), want) == total == need
    finally:
        buf.free()


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("seg", [64, 256])
def test_async_two_calls_before_sync(monkeypatch, seg, w):
    """CLG_F_ASYNC_SLICE: two slice calls back to back, each with runs that share logs, then
    one sync -- the two descriptor sets in flight at once."""
    want = expected(seg)
    need = sum(len(d) for _, _, d in want)
    bufs = [DeviceBuf(need + 64), DeviceBuf(need + 64)]
    try:
        with open_engine(monkeypatch, seg, w, async_slice=True) as eng:
            logs, reqs = staged_engine_logs(eng, seg)
            halves = [list(range(0, len(reqs), 2)), list(range(1, len(reqs), 2))]
            got = []
            for half, buf in zip(halves, bufs):
                got.append(eng.slice_batch([(logs[reqs[k][0]], reqs[k][1], 0) for k in half], out=buf.p.value,
                                           cap=need))
            eng.sync()
            for half, buf, (res, _, total) in zip(halves, bufs, got):
                hw = [want[k] for k in half]
                assert check_results(res, buf.host(), hw) == total == sum(len(d) for _, _, d in hw)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("w", [None, 0, 5])
def test_default_window_cuts_long_logs(monkeypatch, w):
    """16 KiB segments and logs longer than 2 MiB: the default cuts every run that crosses the
    2 MiB mark (0: request order; 5: 27 windows); host output, then device output on the
    asynchronous path."""
    want = expected(BIG_SEG)
    need = sum(len(d) for _, _, d in want)
    with open_engine(monkeypatch, BIG_SEG, w) as eng:
        logs, reqs = staged_engine_logs(eng, BIG_SEG)
        res, out, total = eng.slice_batch([(logs[i], ch, 0) for i, ch, _ in reqs])
        assert check_results(res, out, want) == total == need
    buf = DeviceBuf(need + 64)
    try:
        with open_engine(monkeypatch, BIG_SEG, w, async_slice=True) as eng:
            logs, reqs = staged_engine_logs(eng, BIG_SEG)
            res, _, total = eng.slice_batch([(logs[i], ch, 0) for i, ch, _ in reqs], out=buf.p.value, cap=need)
            eng.sync()
            assert check_results(res, buf.host(), want) == total == need
    finally:
        buf.free()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("seg", [64, 256])
def test_capacity_failure_in_mid_batch(monkeypatch, seg, w, device):
    """A buffer a few bytes short of the whole batch: the requests that no longer fit fail with
    CLG_E_CAPACITY, the others -- before and after them, of the same logs -- are correct and
    packed as if the failed ones were absent, and a failed request's consumer has not moved:
    asked again, it gets its whole delta."""
    want = expected(seg)
    lens = [len(d) for _, _, d in want]
    # room for everything but the largest request that is neither first nor last in the batch
    big = max(range(1, len(lens) - 1), key=lambda k: lens[k])
    cap = sum(lens) - lens[big] + lens[big] // 2
    failed, dst = [], 0
    for k, n in enumerate(lens):
        if dst + n > cap:
            failed.append(k)
        else:
            dst += n
    assert failed and 0 < failed[0] and len(failed) < len(lens) - 1
    buf = DeviceBuf(sum(lens) + 64) if device else None
    try:
        with open_engine(monkeypatch, seg, w) as eng:
            logs, reqs = staged_engine_logs(eng, seg)
            batch = [(logs[i], ch, 0) for i, ch, _ in reqs]
            if device:
                res, _, total = eng.slice_batch(batch, out=buf.p.value, cap=cap)
                eng.sync()
                data = buf.host()
            else:
                res, data, total = eng.slice_batch(batch, cap=cap)
            assert check_results(res, data, want, failed) == total == dst
            for k in failed:
                i, ch, o = reqs[k]
                assert logs[i].consumer_state(ch)[1] == o  # (one epoch from offset 0: the offset in it)
            # again, with room: the failed requests' deltas whole, nothing for the others
            again = [w_ if k in failed else (False, 0, b"") for k, w_ in enumerate(want)]
            if device:
                res, _, total = eng.slice_batch(batch, out=buf.p.value, cap=sum(lens))
                eng.sync()
                data = buf.host()
            else:
                res, data, total = eng.slice_batch(batch)
            assert check_results(res, data, again) == total == sum(lens[k] for k in failed)
    finally:
        if buf:
            buf.free()


@pytest.mark.parametrize("w", WINDOWS)
def test_one_two_and_eight_consumers_alone(monkeypatch, w):
    """Each log's consumers in a batch of their own (1, 2 and 8 runs of one log), seg 64."""
    seg = 64
    want = expected(seg)
    with open_engine(monkeypatch, seg, w) as eng:
        logs, reqs = staged_engine_logs(eng, seg)
        for i in (2, 1, 0):
            ks = [k for k, r in enumerate(reqs) if r[0] == i]
            assert len(ks) == (8, 2, 1)[i]
            res, out, total = eng.slice_batch([(logs[i], reqs[k][1], 0) for k in ks])
            hw = [want[k] for k in ks]
            assert check_results(res, out, hw) == total == sum(len(d) for _, _, d in hw)
