"""GPU: the longest common prefix of log ranges and reference spans (clg_diff_logs,
clonos_amd/csrc/diff.hip).

The oracle is os.path.commonprefix over getDeterminants(start_epoch) and the reference bytes.
Every case runs with host input and with device input (a torch tensor on the engine's device,
exactly as long as the packed spans: nothing behind the last one).
"""
import os

import numpy as np
import pytest
import torch

from clonos_amd import DIFF, CausalLogID, ClonosError, Engine, _lib

pytestmark = pytest.mark.gpu

# Bytes a wave of k_diff_pieces covers per iteration: 64 lanes x 4 windows x 16 bytes, counted
# from the 16-byte-aligned address at or before the piece's first byte.
WAVE_ITER_BYTES = 4096

KINDS = ["host", "device"]


def lcp(a: bytes, b: bytes) -> int:
    return len(os.path.commonprefix([a, b]))


def rows(d):
    assert d.dtype == DIFF
    return [(int(x["lcp"]), int(x["len_log"]), int(x["len_ref"])) for x in d]


def want_rows(log_bytes, ref_bytes):
    return [(lcp(a, b), len(a), len(b)) for a, b in zip(log_bytes, ref_bytes)]


def pack(spans, residues=None, gap_byte=0x5A):
    """The spans in one buffer, span i at an offset of residue residues[i] mod 16 (None: back to
    back); the gaps hold gap_byte."""
    buf = bytearray()
    offs = []
    for i, s in enumerate(spans):
        if residues is not None:
            buf += bytes([gap_byte]) * ((residues[i] - len(buf)) % 16)
        offs.append(len(buf))
        buf += s
    return bytes(buf), np.array(offs, np.uint64), np.array([len(s) for s in spans], np.uint64)


def diff(eng, kind, handles, epochs, buf, offs, lens):
    if kind == "host":
        return rows(eng.diff_logs(handles, epochs, buf, offs, lens))
    dev = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to("cuda:0") if len(buf) else torch.empty(
        0, dtype=torch.uint8, device="cuda:0")
    got = rows(eng.diff_logs(handles, epochs, dev.data_ptr(), offs, lens, device=True))
    torch.cuda.synchronize()
    return got


def flipped(b: bytes, *at, bit=0x01) -> bytes:
    f = bytearray(b)
    for d in at:
        f[d] ^= bit
    return bytes(f)


# ---- every relative alignment ------------------------------------------------------------
LENGTHS = [1, 3, 4, 15, 16, 17, 255, 256, 257, 600]


@pytest.fixture(scope="module")
def aligned_case():
    """160 logs: a leading epoch of s bytes (s in 0..15), then the compared epoch of each length;
    every log is compared with 16 copies of its range, one at every residue mod 16."""
    rng = np.random.default_rng(71)
    logs = []
    for n in LENGTHS:
        for s in range(16):
            logs.append((bytes(rng.integers(0, 256, s, dtype=np.uint8)), bytes(rng.integers(0, 256, n, dtype=np.uint8))))
    which, residues = [], []
    for i in range(len(logs)):
        for r in range(16):
            which.append(i)
            residues.append(r)
    buf, offs, lens = pack([logs[i][1] for i in which], residues)
    assert sorted(set(int(o) % 16 for o in offs)) == list(range(16))
    return logs, which, buf, offs, lens


@pytest.mark.parametrize("kind", KINDS)
def test_every_relative_alignment(aligned_case, kind):
    logs, which, buf, offs, lens = aligned_case
    with Engine(segment_bytes=256, pool_segments=2048) as eng:
        hs = []
        for i, (lead, body) in enumerate(logs):
            log = eng.open_log(CausalLogID.main(1 + i))
            if lead:
                log.appendDeterminant(lead, 0)
            log.appendDeterminant(body, 1)
            hs.append(log.handle)
        got = diff(eng, kind, [hs[i] for i in which], [1] * len(which), buf, offs, lens)
        assert got == [(len(logs[i][1]),) * 3 for i in which]


# ---- every position ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def position_case():
    rng = np.random.default_rng(72)
    lead = bytes(rng.integers(0, 256, 37, dtype=np.uint8))  # the range starts 37 bytes into a segment
    body = bytes(rng.integers(0, 256, 700, dtype=np.uint8))
    return lead, body


@pytest.mark.parametrize("variant", ["one_bit", "second_flip", "bit7"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_position(position_case, kind, variant):
    lead, body = position_case
    n = len(body)
    if variant == "one_bit":
        refs = [flipped(body, d) for d in range(n)]
    elif variant == "bit7":
        refs = [flipped(body, d, bit=0x80) for d in range(n)]
    else:  # a second flip at some d' > d (none behind the last byte)
        refs = [flipped(body, d, *([d + 1 + (7 * d) % (n - d - 1)] if d < n - 1 else [])) for d in range(n)]
    buf, offs, lens = pack(refs)
    with Engine(segment_bytes=256, pool_segments=256) as eng:
        log = eng.open_log(CausalLogID.main(1))
        log.appendDeterminant(lead, 0)
        log.appendDeterminant(body, 1)
        got = diff(eng, kind, [log.handle] * n, [1] * n, buf, offs, lens)
        assert got == want_rows([body] * n, refs)
        assert [g[0] for g in got] == list(range(n))


# ---- pieces longer than one wave iteration ---------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_pieces_longer_than_a_wave_iteration(kind):
    rng = np.random.default_rng(73)
    seg = 16384
    lead = bytes(rng.integers(0, 256, 5, dtype=np.uint8))
    body = bytes(rng.integers(0, 256, 100_003, dtype=np.uint8))
    first_piece = seg - len(lead)  # the range's bytes in its first segment
    at = {0, len(body) - 1, first_piece, first_piece + seg - 1}  # ... and the second piece's first and last byte
    for k in range(1, first_piece // WAVE_ITER_BYTES + 1):
        for base in (k * WAVE_ITER_BYTES, k * WAVE_ITER_BYTES - len(lead)):  # of the range / of the wave's windows
            at |= {base - 1, base, base + 1}
    at = sorted(at)
    refs = [body] + [flipped(body, d) for d in at]
    buf, offs, lens = pack(refs, residues=[(3 * i) % 16 for i in range(len(refs))])
    with Engine(segment_bytes=seg, pool_segments=64, timing=True) as eng:
        log = eng.open_log(CausalLogID.main(1))
        log.appendDeterminant(lead, 0)
        for k in range(0, len(body), 1 << 15):
            log.appendDeterminant(body[k:k + (1 << 15)], 1)
        eng.sync()
        eng.kernel_stats_reset()
        got = diff(eng, kind, [log.handle] * len(refs), [1] * len(refs), buf, offs, lens)
        assert got == want_rows([body] * len(refs), refs)
        assert [g[0] for g in got] == [len(body)] + at
        st = eng.kernel_stats()["log_diff"]
        assert st["launches"] == 1 and st["bytes"] == 2 * len(body) * len(refs)


# ---- clipping ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 300, 513])
@pytest.mark.parametrize("kind", KINDS)
def test_clipping(kind, n):
    rng = np.random.default_rng(74 + n)
    a = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    b = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    b = bytes([a[-1] ^ 0xFF]) + b[1:]  # b's first byte is not a's last
    with Engine(segment_bytes=256, pool_segments=256) as eng:
        la, lb = eng.open_log(CausalLogID.main(1)), eng.open_log(CausalLogID.main(2))
        la.appendDeterminant(b"\x07" * 3, 0)
        la.appendDeterminant(a, 1)
        lb.appendDeterminant(b, 1)
        # the reference one byte short, a different byte right behind it in the buffer (b's first)
        refs = [a[:-1], b, a, b + bytes([a[0] ^ 1]), a + b"\x99"]
        hs = [la.handle, lb.handle, la.handle, lb.handle, la.handle]
        buf, offs, lens = pack(refs)  # back to back
        got = diff(eng, kind, hs, [1] * len(hs), buf, offs, lens)
        assert got == [(n - 1, n, n - 1), (n, n, n), (n, n, n), (n, n, n + 1), (n, n, n + 1)]
        # overlapping spans of one buffer: a's reference continued into b's bytes
        got = diff(eng, kind, [la.handle], [1], buf, offs[2:3], [n + 3])
        assert got == [(n, n, n + 3)]


@pytest.mark.parametrize("kind", KINDS)
def test_empty_sides(kind):
    with Engine(segment_bytes=256, pool_segments=256) as eng:
        job = eng.open_job((7, 7), sharing_depth=0)
        d0 = eng.open_log(CausalLogID.main(4), job)
        d0.appendDeterminant(b"\x00\x01", 0)
        empty = eng.open_log(CausalLogID.main(5))
        full = eng.open_log(CausalLogID.main(6))
        full.appendDeterminant(b"\x00\x02\x00\x03", 0)
        hs = [full.handle, empty.handle, d0.handle, empty.handle, d0.handle, full.handle]
        refs = [b"", b"\x00\x02", b"\x00\x01", b"", b"", b"\x00\x02\x00\x03"]
        buf, offs, lens = pack(refs)
        got = diff(eng, kind, hs, [0] * len(hs), buf, offs, lens)
        assert got == [(0, 4, 0), (0, 0, 2), (0, 0, 2), (0, 0, 0), (0, 0, 0), (4, 4, 4)]
        # no log with a byte, and nothing at all
        assert diff(eng, kind, [empty.handle, d0.handle], [0, 0], b"\x01\x02", [0, 1], [1, 1]) == [(0, 0, 1), (0, 0, 1)]
        assert diff(eng, kind, [empty.handle], [0], b"", [0], [0]) == [(0, 0, 0)]
        assert len(eng.diff_logs([], [], b"", [], [])) == 0


# ---- request handling ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_repeated_and_shuffled_requests(kind):
    rng = np.random.default_rng(75)
    with Engine(segment_bytes=256, pool_segments=4096) as eng:
        logs, data = [], []
        for i in range(120):
            b = bytes(rng.integers(0, 256, int(rng.integers(1, 700)), dtype=np.uint8))
            log = eng.open_log(CausalLogID.main(100 + i))
            log.appendDeterminant(b, 0)
            logs.append(log)
            data.append(b)
        pick = np.concatenate([rng.permutation(120), rng.integers(0, 120, 40)])
        refs = []
        for j, i in enumerate(pick):
            b = data[i]
            m = j % 4
            if m == 1:
                b = flipped(b, int(rng.integers(len(b))), bit=0x10)
            elif m == 2:
                b = b[:int(rng.integers(len(b)))]
            elif m == 3:
                b = b + b"\x01\x02\x03"
            refs.append(b)
        buf, offs, lens = pack(refs)
        got = diff(eng, kind, [logs[i].handle for i in pick], np.zeros(len(pick), np.int64), buf, offs, lens)
        assert got == want_rows([data[i] for i in pick], refs)


@pytest.mark.parametrize("kind", KINDS)
def test_unflushed_append_is_seen(kind):
    with Engine(segment_bytes=256, pool_segments=256) as eng:
        log = eng.open_log(CausalLogID.main(3))
        first = (b"\x01" + bytes(range(8))) * 40
        log.appendDeterminant(first, 0)
        assert diff(eng, kind, [log.handle], [0], first, [0], [len(first)]) == [(len(first),) * 3]
        more = b"\x00\x09" + b"\x01" + bytes(range(8, 16))
        log.appendDeterminant(more, 0)  # staged: nothing has flushed it yet
        n = len(first + more)
        assert diff(eng, kind, [log.handle], [0], first + more, [0], [n]) == [(n, n, n)]
        assert diff(eng, kind, [log.handle], [0], first + flipped(more, 1), [0], [n]) == [(len(first) + 1, n, n)]


def test_unknown_handle_and_oversized_span():
    with Engine(segment_bytes=256, pool_segments=64) as eng:
        log = eng.open_log(CausalLogID.main(1))
        log.appendDeterminant(b"\x00\x01", 0)
        with pytest.raises(ClonosError) as ei:
            eng.diff_logs([log.handle, 12345], [0, 0], b"\x00\x01", [0, 0], [2, 2])
        assert ei.value.status == _lib.CLG_E_NO_LOG
        dev = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(ClonosError) as ei:
            eng.diff_logs([log.handle], [0], dev.data_ptr(), [0], [1 << 32], device=True)  # refused before any read
        assert ei.value.status == _lib.CLG_E_INVALID_ARG


@pytest.mark.parametrize("kind", KINDS)
def test_after_a_truncation(kind):
    rng = np.random.default_rng(76)
    e0 = bytes(rng.integers(0, 256, 701, dtype=np.uint8))
    e1 = bytes(rng.integers(0, 256, 903, dtype=np.uint8))
    e2 = bytes(rng.integers(0, 256, 500, dtype=np.uint8))
    with Engine(segment_bytes=256, pool_segments=256) as eng:
        log = eng.open_log(CausalLogID.main(2))
        for ep, b in enumerate([e0, e1, e2]):
            log.appendDeterminant(b, ep)
        eng.diff_logs([log.handle], [0], b"", [0], [0])  # (flushes)
        log.notifyCheckpointComplete(1)  # drops epoch 0's whole segments: the log starts mid-segment
        assert log.state()["writer"] < len(e0 + e1 + e2)
        assert log.getDeterminants(1) == e1 + e2
        refs = [e1 + e2, flipped(e1 + e2, 1000), e2, flipped(e2, 0, bit=0x80), e1]
        buf, offs, lens = pack(refs, residues=[1, 6, 11, 0, 13])
        got = diff(eng, kind, [log.handle] * 5, [1, 1, 2, 2, 1], buf, offs, lens)
        assert got == want_rows([e1 + e2, e1 + e2, e2, e2, e1 + e2], refs)
        assert got[1][0] == 1000 and got[3][0] == 0 and got[4] == (len(e1), len(e1 + e2), len(e1))
