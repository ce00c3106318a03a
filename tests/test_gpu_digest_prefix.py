"""GPU: prefix digests (clg_digest_prefixes / clg_digest_epochs, clonos_amd/csrc/digest.hip).

The reference is the definition restated here with Python integers (not taken from
clonos_amd): p = 2^61 - 1, R = 2654435761, little-endian u32 words zero-padded past the end,
h = (h * R + w) mod p per word; the row of a cut c over a range b of n bytes is
{hash(b[:min(c, n)]), min(c, n)}.  Equality is exact.
"""
import numpy as np
import pytest

from clonos_amd import DIGEST, CausalLogID, ClonosError, Engine, _lib

pytestmark = pytest.mark.gpu

P = (1 << 61) - 1
R = 2654435761


def ref_digest(b: bytes):
    h = 0
    for k in range(0, len(b), 4):
        h = (h * R + int.from_bytes(b[k:k + 4].ljust(4, b"\0"), "little")) % P
    return h, len(b)


def ref_every_byte(b: bytes):
    """ref_digest(b[:c]) for c = 0 .. len(b), the definition word by word (h before the word
    that holds byte c - 1, then that word cut at c)."""
    out, h = [(0, 0)], 0
    for k in range(0, len(b), 4):
        for c in range(k + 1, min(k + 4, len(b)) + 1):
            out.append(((h * R + int.from_bytes(b[k:c], "little")) % P, c))
        h = (h * R + int.from_bytes(b[k:k + 4].ljust(4, b"\0"), "little")) % P
    return out


def ref_rows(b: bytes, cuts):
    return [ref_digest(b[:min(int(c), len(b))]) for c in cuts]


def rows(d):
    assert d.dtype == DIGEST
    return [(int(x["hash"]), int(x["len"])) for x in d]


def order(v):
    return bytes([0, v & 0xFF])  # OrderDeterminant: tag 0, one byte


def timestamp(v):
    return bytes([1]) + int(v).to_bytes(8, "big")  # TimestampDeterminant: tag 1, eight bytes


def mixed_records(rng, n_bytes_at_least):
    out = bytearray()
    while len(out) < n_bytes_at_least:
        out += order(int(rng.integers(256))) if rng.random() < 0.5 else timestamp(int(rng.integers(1 << 62)))
    return bytes(out)


@pytest.fixture(scope="module")
def three_epochs():
    """Mixed 2- and 9-byte records over epochs 0..2: the epoch starts are odd and no multiple
    of 16, the total length is no multiple of 4."""
    rng = np.random.default_rng(61)
    e0 = mixed_records(rng, 700)
    if len(e0) % 2 == 0:
        e0 += timestamp(5)
    e1 = mixed_records(rng, 900)
    while (len(e0) + len(e1)) % 2 == 0 or (len(e0) + len(e1)) % 16 == 0:
        e1 += timestamp(6)
    e2 = mixed_records(rng, 500)
    while (len(e0) + len(e1) + len(e2)) % 4 == 0:
        e2 += order(7)
    return [e0, e1, e2]


@pytest.fixture(scope="module")
def every_byte_want(three_epochs):
    e0, e1, e2 = three_epochs
    whole = e0 + e1 + e2
    return [ref_every_byte(whole[s:]) for s in (0, len(e0), len(e0) + len(e1))]


def fill(log, epochs):
    for ep, b in enumerate(epochs):
        log.appendDeterminant(b, ep)


def test_reference_every_byte_restates_the_definition():
    rng = np.random.default_rng(60)
    b = bytes(rng.integers(0, 256, 41, dtype=np.uint8))
    assert ref_every_byte(b) == [ref_digest(b[:c]) for c in range(len(b) + 1)]


@pytest.mark.parametrize("segment_bytes,pool_segments", [(256, 1024), (16384, 64)])
def test_every_byte(three_epochs, every_byte_want, segment_bytes, pool_segments):
    """Every lead phase, cuts inside words that straddle a segment boundary, one-byte stretches
    and more than 64 cuts per request in the chain."""
    e0, e1, e2 = three_epochs
    whole = e0 + e1 + e2
    starts = [0, len(e0), len(e0) + len(e1)]
    assert 2000 < len(whole) < 2300 and starts[1] % 2 == 1 and starts[2] % 2 == 1 and len(whole) % 4
    with Engine(segment_bytes=segment_bytes, pool_segments=pool_segments) as eng:
        log = eng.open_log(CausalLogID.main(1))
        fill(log, three_epochs)
        cuts = [np.arange(len(whole) - s + 1) for s in starts]
        got, first = eng.digest_prefixes([log.handle] * 3, [0, 1, 2], cuts)
        assert list(first) == list(np.cumsum([0] + [len(c) for c in cuts]))
        got = rows(got)
        for i in range(3):
            assert got[int(first[i]):int(first[i + 1])] == every_byte_want[i], i
        # the (first, flat) form of the same request
        again, _ = eng.digest_prefixes([log.handle] * 3, [0, 1, 2], (first, np.concatenate(cuts)))
        assert rows(again) == got


def test_clamping_duplicates_and_order(three_epochs):
    e0, e1, e2 = three_epochs
    whole = e0 + e1 + e2
    n = len(whole)
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(2))
        fill(log, three_epochs)
        cuts = [0, 0, 5, 5, n, n + 1, (1 << 32) - 1]
        got, _ = eng.digest_prefixes([log.handle], [0], [cuts])
        got = rows(got)
        assert got == ref_rows(whole, cuts)
        assert got[0] == got[1] == (0, 0) and got[5][1] == got[6][1] == n
        assert got[4] == rows(eng.digest_logs([log.handle], [0]))[0]
        tail = whole[len(e0):]
        got, _ = eng.digest_prefixes([log.handle, log.handle], [1, 0], [[len(tail)], [n]])
        assert rows(got) == rows(eng.digest_logs([log.handle, log.handle], [1, 0])) == [ref_digest(tail),
                                                                                       ref_digest(whole)]
        for bad in ([[5, 4]], [[0, 9, 9, 8]]):
            with pytest.raises(ClonosError) as ei:
                eng.digest_prefixes([log.handle], [0], bad)
            assert ei.value.status == _lib.CLG_E_INVALID_ARG
        with pytest.raises(ClonosError) as ei:  # the second request's cuts decrease
            eng.digest_prefixes([log.handle, log.handle], [0, 0], [[1, 2], [3, 1]])
        assert ei.value.status == _lib.CLG_E_INVALID_ARG and "request 1" in str(ei.value)
        got, _ = eng.digest_prefixes([log.handle, log.handle], [0, 0], [[7, 9], [3, 8]])  # (each request on its own)
        assert rows(got) == ref_rows(whole, [7, 9, 3, 8])


def test_short_lengths_at_every_byte():
    rng = np.random.default_rng(62)
    lengths = list(range(10)) + [255, 256, 257, 513]
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        logs, data = [], []
        for i, n in enumerate(lengths):
            # a 3-byte epoch 0 in front: epoch 1 starts at an odd physical offset
            b = bytes(rng.integers(0, 256, n, dtype=np.uint8))
            log = eng.open_log(CausalLogID.main(10 + i))
            log.appendDeterminant(b"\x00\x01\x02", 0)
            if n:
                log.appendDeterminant(b, 1)
            logs.append(log)
            data.append(b if n else b"\x00\x01\x02")  # (an absent epoch 1 answers from the earliest epoch)
        cuts = [np.arange(len(b) + 1) for b in data]
        got, first = eng.digest_prefixes([l.handle for l in logs], [1] * len(logs), cuts)
        got = rows(got)
        for i, b in enumerate(data):
            assert got[int(first[i]):int(first[i + 1])] == ref_every_byte(b), lengths[i]


def test_many_small_logs_shuffled_with_duplicates():
    rng = np.random.default_rng(63)
    with Engine(segment_bytes=256, pool_segments=4096) as eng:
        job = eng.open_job((7, 7), sharing_depth=0)
        d0 = eng.open_log(CausalLogID.main(4), job)
        d0.appendDeterminant(order(1), 0)
        logs, data = [d0, eng.open_log(CausalLogID.main(5))], [b"", b""]  # a depth-0 log, an empty range
        for i in range(200):
            b = mixed_records(rng, int(rng.integers(1, 700)))
            log = eng.open_log(CausalLogID.main(100 + i))
            log.appendDeterminant(b, 0)
            logs.append(log)
            data.append(b)
        pick = np.concatenate([[0, 1], rng.permutation(len(logs)), rng.integers(0, len(logs), 40)])
        cuts = [np.sort(rng.integers(0, len(data[i]) + 20, int(rng.integers(0, 6)))) for i in pick]
        cuts[0], cuts[1] = np.array([0, 1, 9]), np.array([0, 3])
        assert any(len(c) == 0 for c in cuts)
        got, first = eng.digest_prefixes([logs[i].handle for i in pick], np.zeros(len(pick), np.int64), cuts)
        got = rows(got)
        assert got[:5] == [(0, 0)] * 5
        for j, i in enumerate(pick):
            assert got[int(first[j]):int(first[j + 1])] == ref_rows(data[i], cuts[j]), j
        # requests without cuts only, and no requests at all
        got, first = eng.digest_prefixes([logs[2].handle, logs[3].handle], [0, 0], [[], []])
        assert len(got) == 0 and list(first) == [0, 0, 0]
        got, first = eng.digest_prefixes([], [], [])
        assert len(got) == 0 and list(first) == [0]
        with pytest.raises(ClonosError) as ei:
            eng.digest_prefixes([0xFFFFFF], [0], [[1]])
        assert ei.value.status == _lib.CLG_E_NO_LOG


def test_after_checkpoint_complete(three_epochs):
    e0, e1, e2 = three_epochs
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(2))
        fill(log, three_epochs)
        eng.digest_logs([log.handle], [0])  # (flushes)
        log.notifyCheckpointComplete(1)  # drops epoch 0's whole segments: a nonzero physical start
        assert log.state()["writer"] < len(e0 + e1 + e2)
        cuts = [[1, 2, 3, 250, 255, 256, 257, 258, len(e1), len(e1 + e2)], [0, 6, 7, len(e2) - 1, len(e2)]]
        got, first = eng.digest_prefixes([log.handle, log.handle], [1, 2], cuts)
        assert rows(got) == ref_rows(e1 + e2, cuts[0]) + ref_rows(e2, cuts[1])


def test_unflushed_appends_are_included():
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(3))
        first = timestamp(11) * 40
        log.appendDeterminant(first, 0)
        cuts = [7, len(first), len(first) + 5, 1000]
        got, _ = eng.digest_prefixes([log.handle], [0], [cuts])
        assert rows(got) == ref_rows(first, cuts)
        more = order(9) + timestamp(12)
        log.appendDeterminant(more, 0)  # staged: nothing has flushed it yet
        got, _ = eng.digest_prefixes([log.handle], [0], [cuts])
        assert rows(got) == ref_rows(first + more, cuts)


def test_long_stretches_and_kernel_stat():
    """Stretches of many 16 KiB segments: a lane takes several windows with a nonzero lead."""
    rng = np.random.default_rng(64)
    b = bytes(rng.integers(0, 256, 1 << 20, dtype=np.uint8))
    cuts = [int(c) for c in rng.integers(16, len(b) - 16, 7)]
    cuts = sorted(c - c % 4 + j % 4 for j, c in enumerate(cuts)) + [len(b)]  # a cut at each residue mod 4
    assert {c % 4 for c in cuts[:-1]} == {0, 1, 2, 3} and max(np.diff([0] + cuts)) > 4 * 16384
    want = ref_rows(b, cuts)
    with Engine(segment_bytes=16384, pool_segments=128, timing=True) as eng:
        log = eng.open_log(CausalLogID.main(7))
        for k in range(0, len(b), 1 << 16):
            log.appendDeterminant(b[k:k + (1 << 16)], 0)
        eng.sync()
        eng.kernel_stats_reset()
        got, _ = eng.digest_prefixes([log.handle], [0], [cuts])
        assert rows(got) == want
        st = eng.kernel_stats()
        assert "log_digest_prefix" in st and "log_digest" not in st
        assert st["log_digest_prefix"]["bytes"] == len(b) and st["log_digest_prefix"]["launches"] == 1
        # bytes up to the largest cut are read, once, however many cuts lie below it
        got, _ = eng.digest_prefixes([log.handle], [0], [[3, 3, 70001, 70001, 70002]])
        assert rows(got) == ref_rows(b, [3, 3, 70001, 70001, 70002])
        assert eng.kernel_stats()["log_digest_prefix"]["bytes"] == len(b) + 70002
        assert rows(eng.digest_logs([log.handle], [0])) == [want[-1]]


def epoch_ends(log, start_epoch):
    """(ids, ends relative to the range's start) of getDeterminants(start_epoch), from log.state()."""
    st = log.state()
    eps = sorted(st["epochs"])
    if start_epoch in dict(eps):
        eps = [(i, o) for i, o in eps if i >= start_epoch]
    s = eps[0][1]
    offs = [o for _, o in eps[1:]] + [st["writer"]]
    return [i for i, _ in eps], [o - s for o in offs]


def test_digest_epochs(three_epochs):
    e0, e1, e2 = three_epochs
    whole = e0 + e1 + e2
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(1))
        fill(log, three_epochs)
        other = eng.open_log(CausalLogID.main(2))
        other.appendDeterminant(e1, 4)
        other.appendDeterminant(e2, 7)
        empty = eng.open_log(CausalLogID.main(3))
        job = eng.open_job((7, 7), sharing_depth=0)
        d0 = eng.open_log(CausalLogID.main(4), job)
        d0.appendDeterminant(order(1), 0)
        logs = [log, other, log, empty, log, d0, log]
        eps = [0, 0, 1, 0, 2, 0, 9]  # (epoch 9 is absent: from the earliest)
        first, ids, got = eng.digest_epochs([l.handle for l in logs], eps)
        got = rows(got)
        assert list(first) == [0, 3, 5, 7, 7, 8, 8, 11]
        assert list(ids) == [0, 1, 2, 4, 7, 1, 2, 2, 0, 1, 2]
        assert got[0:3] == ref_rows(whole, [len(e0), len(e0 + e1), len(whole)])
        assert got[3:5] == ref_rows(e1 + e2, [len(e1), len(e1 + e2)])
        assert got[5:7] == ref_rows(e1 + e2, [len(e1), len(e1 + e2)])
        assert got[7:8] == [ref_digest(e2)] and got[8:11] == got[0:3]
        # the same rows from digest_prefixes at the epoch ends that log.state() gives
        for j in (0, 1, 2, 4, 6):
            e_ids, ends = epoch_ends(logs[j], eps[j])
            assert list(ids[int(first[j]):int(first[j + 1])]) == e_ids
            pre, _ = eng.digest_prefixes([logs[j].handle], [eps[j]], [ends])
            assert rows(pre) == got[int(first[j]):int(first[j + 1])]
        # the last row of a request is digest_logs' row
        last = rows(eng.digest_logs([l.handle for l in (log, other, log, log)], [0, 0, 1, 2]))
        assert [got[2], got[4], got[6], got[7]] == last


def test_digest_epochs_empty_epoch_and_capacity(three_epochs):
    import ctypes as C
    e0, e1, e2 = three_epochs
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(1))
        log.appendDeterminant(e0, 0)
        log.appendDeterminant(e1, 2)
        log.appendDeterminant(b"", 3)  # opens epoch 3 with nothing in it
        log.appendDeterminant(e2, 5)
        first, ids, got = eng.digest_epochs([log.handle], [0])
        got = rows(got)
        e_ids, ends = epoch_ends(log, 0)
        assert list(ids) == e_ids and len(got) == len(e_ids)
        assert got == ref_rows(e0 + e1 + e2, ends)
        assert e_ids == [0, 2, 3, 5] and ends == [len(e0), len(e0 + e1), len(e0 + e1), len(e0 + e1 + e2)]
        assert got[2] == got[1]  # an empty epoch repeats the row before it
        # sizes only, and too small a capacity
        h = np.array([log.handle, log.handle], np.uint32)
        ep = np.array([0, 2], np.int64)
        f = np.zeros(3, np.uint64)
        total = C.c_uint64(0)
        lib = _lib.lib
        assert lib.clg_digest_epochs(eng._h, h.ctypes.data, ep.ctypes.data, 2, 0, f.ctypes.data, None, None,
                                     C.byref(total)) == _lib.CLG_OK
        n0 = len(e_ids)
        assert total.value == 2 * n0 - 1 and list(f) == [0, n0, 2 * n0 - 1]
        out = np.zeros(total.value, DIGEST)
        eid = np.zeros(total.value, np.int64)
        total2 = C.c_uint64(0)
        assert lib.clg_digest_epochs(eng._h, h.ctypes.data, ep.ctypes.data, 2, total.value - 1, f.ctypes.data,
                                     eid.ctypes.data, out.ctypes.data, C.byref(total2)) == _lib.CLG_E_CAPACITY
        assert total2.value == total.value and not out["len"].any()
        assert lib.clg_digest_epochs(eng._h, h.ctypes.data, ep.ctypes.data, 2, total.value, f.ctypes.data,
                                     eid.ctypes.data, out.ctypes.data, C.byref(total2)) == _lib.CLG_OK
        assert rows(out)[:n0] == got and list(eid[:n0]) == e_ids
