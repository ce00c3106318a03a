"""GPU: device-side log digests (clg_digest_logs / clg_digest_spans, clonos_amd/csrc/digest.hip).

The reference is the definition restated here with Python integers (not taken from
clonos_amd): p = 2^61 - 1, R = 2654435761, little-endian u32 words zero-padded past the end,
h = (h * R + w) mod p per word; a digest is {hash, len} and both must match.
"""
import numpy as np
import pytest
import torch

from clonos_amd import DIGEST, CausalLogID, Engine

pytestmark = pytest.mark.gpu

P = (1 << 61) - 1
R = 2654435761


def ref_digest(b: bytes):
    h = 0
    for k in range(0, len(b), 4):
        h = (h * R + int.from_bytes(b[k:k + 4].ljust(4, b"\0"), "little")) % P
    return h, len(b)


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
        e0 += timestamp(5)  # an odd start for epoch 1
    e1 = mixed_records(rng, 900)
    while (len(e0) + len(e1)) % 2 == 0 or (len(e0) + len(e1)) % 16 == 0:
        e1 += timestamp(6)
    e2 = mixed_records(rng, 500)
    while (len(e0) + len(e1) + len(e2)) % 4 == 0:
        e2 += order(7)
    return [e0, e1, e2]


def fill(log, epochs):
    for ep, b in enumerate(epochs):
        log.appendDeterminant(b, ep)


def test_log_digest_from_each_epoch(three_epochs):
    e0, e1, e2 = three_epochs
    whole = e0 + e1 + e2
    starts = [0, len(e0), len(e0) + len(e1)]
    assert starts[1] % 2 == 1 and starts[2] % 2 == 1 and starts[1] % 16 and starts[2] % 16 and len(whole) % 4
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(1))
        fill(log, three_epochs)
        got = rows(eng.digest_logs([log.handle] * 3, [0, 1, 2]))
        want = [ref_digest(whole[s:]) for s in starts]
        assert got == want
        for ep, s in enumerate(starts):
            assert log.getDeterminants(ep) == whole[s:]  # what the digest stands for
        # the same bytes as flat spans, from host and from device memory at an odd offset
        pad = b"\xA5" * 37
        host = pad + whole
        offs = [len(pad) + s for s in starts]
        lens = [len(whole) - s for s in starts]
        assert rows(eng.digest_spans(host, offs, lens)) == want
        dev = torch.from_numpy(np.frombuffer(host, np.uint8).copy()).to("cuda:0")
        assert rows(eng.digest_spans(dev.data_ptr(), offs, lens, device=True)) == want
        assert rows(eng.digest_spans(dev.data_ptr() + 1, [o - 1 for o in offs], lens, device=True)) == want
    # the digest does not depend on segmentation
    with Engine(segment_bytes=16384, pool_segments=64) as eng:
        log = eng.open_log(CausalLogID.main(1))
        fill(log, three_epochs)
        assert rows(eng.digest_logs([log.handle] * 3, [0, 1, 2])) == want


def test_lengths_around_words_and_segments():
    rng = np.random.default_rng(62)
    lengths = list(range(10)) + [255, 256, 257, 513]
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        logs, data = [], []
        for i, n in enumerate(lengths):
            # a 3-byte epoch 0 in front: epoch 1 starts at an odd physical offset, so its
            # logical words straddle the 256-byte segment boundaries
            b = bytes(rng.integers(0, 256, n, dtype=np.uint8))
            log = eng.open_log(CausalLogID.main(10 + i))
            log.appendDeterminant(b"\x00\x01\x02", 0)
            if n:
                log.appendDeterminant(b, 1)
            logs.append(log)
            data.append(b)
        got = rows(eng.digest_logs([l.handle for l in logs], [1] * len(logs)))
        # (an absent epoch 1 -- the length-0 case -- answers from the earliest epoch)
        want = [ref_digest(b) if b else ref_digest(b"\x00\x01\x02") for b in data]
        assert got == want
        whole = rows(eng.digest_logs([l.handle for l in logs], [0] * len(logs)))
        assert whole == [ref_digest(b"\x00\x01\x02" + b) for b in data]
        flat = b"".join(data)
        offs = np.cumsum([0] + lengths[:-1])
        assert rows(eng.digest_spans(flat, offs, lengths)) == [ref_digest(b) for b in data]


def test_after_checkpoint_complete(three_epochs):
    e0, e1, e2 = three_epochs
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(2))
        fill(log, three_epochs)
        eng.digest_logs([log.handle], [0])  # (flushes)
        log.notifyCheckpointComplete(1)  # drops epoch 0's whole segments: a nonzero physical start
        assert log.state()["writer"] < len(e0 + e1 + e2)  # whole segments left: physical offsets moved
        assert log.getDeterminants(1) == e1 + e2
        assert rows(eng.digest_logs([log.handle, log.handle], [1, 2])) == [ref_digest(e1 + e2), ref_digest(e2)]


def test_unflushed_appends_are_included():
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        log = eng.open_log(CausalLogID.main(3))
        first = timestamp(11) * 40
        log.appendDeterminant(first, 0)
        assert rows(eng.digest_logs([log.handle], [0])) == [ref_digest(first)]
        more = order(9) + timestamp(12)
        log.appendDeterminant(more, 0)  # staged: nothing has flushed it yet
        assert rows(eng.digest_logs([log.handle], [0])) == [ref_digest(first + more)]


def test_depth0_and_empty():
    with Engine(segment_bytes=256, pool_segments=1024) as eng:
        job = eng.open_job((7, 7), sharing_depth=0)
        d0 = eng.open_log(CausalLogID.main(4), job)
        d0.appendDeterminant(order(1), 0)
        empty = eng.open_log(CausalLogID.main(5))
        full = eng.open_log(CausalLogID.main(6))
        full.appendDeterminant(order(2), 0)
        got = rows(eng.digest_logs([d0.handle, empty.handle, full.handle], [0, 0, 0]))
        assert got == [(0, 0), (0, 0), ref_digest(order(2))]
        assert rows(eng.digest_logs([d0.handle, empty.handle], [0, 3])) == [(0, 0), (0, 0)]
        assert len(eng.digest_logs([], [])) == 0


def test_many_small_logs_shuffled_with_duplicates():
    rng = np.random.default_rng(63)
    with Engine(segment_bytes=256, pool_segments=4096) as eng:
        logs, data = [], []
        for i in range(300):
            b = mixed_records(rng, int(rng.integers(1, 700)))
            log = eng.open_log(CausalLogID.main(100 + i))
            log.appendDeterminant(b, 0)
            logs.append(log)
            data.append(b)
        pick = np.concatenate([rng.permutation(300), rng.integers(0, 300, 60)])
        got = rows(eng.digest_logs([logs[i].handle for i in pick], np.zeros(len(pick), np.int64)))
        assert got == [ref_digest(data[i]) for i in pick]


def test_one_mebibyte_log_and_kernel_stat():
    rng = np.random.default_rng(64)
    b = bytes(rng.integers(0, 256, 1 << 20, dtype=np.uint8))
    with Engine(segment_bytes=16384, pool_segments=128, timing=True) as eng:
        log = eng.open_log(CausalLogID.main(7))
        for k in range(0, len(b), 1 << 16):
            log.appendDeterminant(b[k:k + (1 << 16)], 0)
        eng.sync()
        eng.kernel_stats_reset()
        assert rows(eng.digest_logs([log.handle], [0])) == [ref_digest(b)]  # 64 pieces, exponents to 2^18
        st = eng.kernel_stats()
        assert "log_digest" in st and st["log_digest"]["bytes"] == len(b) and st["log_digest"]["launches"] == 1
        assert rows(eng.digest_spans(b, [0, 3], [len(b), len(b) - 3])) == [ref_digest(b), ref_digest(b[3:])]
        assert eng.kernel_stats()["log_digest"]["bytes"] == 3 * len(b) - 3


def test_hash_zero_vector():
    v = bytes.fromhex("39efc63396a82399")  # a * R + b == p exactly: an unreduced result would be p
    with Engine(segment_bytes=256, pool_segments=64) as eng:
        log = eng.open_log(CausalLogID.main(8))
        log.appendDeterminant(v, 0)
        assert rows(eng.digest_logs([log.handle], [0])) == [(0, 8)]
        assert rows(eng.digest_spans(v, [0], [8])) == [(0, 8)]


def test_span_of_4gib_is_invalid():
    from clonos_amd import ClonosError, _lib
    with Engine(segment_bytes=256, pool_segments=64) as eng:
        with pytest.raises(ClonosError) as ei:
            dev = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
            eng.digest_spans(dev.data_ptr(), [0], [1 << 32], device=True)  # refused before any read
        assert ei.value.status == _lib.CLG_E_INVALID_ARG
