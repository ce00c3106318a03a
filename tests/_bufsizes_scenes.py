"""Scenes of the subpartition recovery buffers' edge tests (test_gpu_bufsizes_edges.py), free of
engine calls: buffers of 5-byte BufferBuilt records [07][size i32 BE] whose sizes cover the whole
int32 range, span lengths around the 256-record chunk of k_bufsizes, records that are not a
BufferBuilt at the chunk seams, and span counts around the 64 of k_bufsizes_classify's workgroup.
test_bufsizes_edges_scene.py checks the coverage these scenes claim without a GPU.

The reference is oracle/response_ref.buffer_sizes (SubpartitionRecoveryThread.run's decodeNext
loop); expected() gives its answer as (sizes, status, err_off, err_tag).
"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import response_ref as R  # noqa: E402  (checker)

CHUNK = 256    # records per workgroup of k_bufsizes (kRecPerChunk, kBufThreads)
CLASSIFY = 64  # spans per workgroup of k_bufsizes_classify
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# the whole int32 range: its ends, a value whose four bytes differ, the sign bit alone, and
# values with only one byte set (the top byte among them)
VALUES = [INT32_MIN, -1, 0, 1, INT32_MAX, 0x01020304, 0x80000000 - (1 << 32), 0x01000000, 0x7F000000,
          0xFF000000 - (1 << 32), 0x00FF0000, 0x0000FF00, 0x000000FF, 0x80C07F01 - (1 << 32)]


def values(n, seed):
    """n sizes: VALUES in turn at the start, then draws from the whole int32 range."""
    r = np.random.default_rng(seed).integers(INT32_MIN, INT32_MAX + 1, n)
    return [VALUES[i] if i < len(VALUES) else int(r[i]) for i in range(n)]


def bb(vals):
    return b"".join(b"\x07" + struct.pack(">i", v) for v in vals)


def good(n, seed):
    return bb(values(n, seed))


def expected(buf):
    """(sizes before the end or the error, status, err_off, err_tag) of the reference loop."""
    try:
        return R.buffer_sizes(buf), 0, -1, -1
    except ValueError as e:
        (st, off, tag), before = e.args
        return before, st, off, tag


# ---- lengths ------------------------------------------------------------------------------------------
TAILS = {"truncated": b"\x07\x01\x02\x03", "order": b"\x00\x05\x07\x01"}  # cut to 1..4 bytes


def length_spans():
    """(name, bytes): whole records around the chunk seam, and partial tails of 1..4 bytes that
    are a cut BufferBuilt (07 ..: truncated) or start with an Order (00 xx: a record that decodes
    and is not a BufferBuilt; 00 alone: truncated)."""
    out = [("records_7", good(7, 99)), ("empty", b"")]
    for r in range(1, 5):
        for t, tail in TAILS.items():
            out.append((f"only_{t}_{r}", tail[:r]))
    for j, n in enumerate((1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK)):
        out.append((f"records_{n}", good(n, 100 + j)))
    for r in range(1, 5):
        for t, tail in TAILS.items():
            out.append((f"chunk_plus_{t}_{r}", good(CHUNK, 110 + r) + tail[:r]))
    out.append((f"records_{2 * CHUNK + 1}_plus_3", good(2 * CHUNK + 1, 120) + TAILS["truncated"][:3]))
    return out


# ---- the first record that is not a BufferBuilt ----------------------------------------------------------
BAD_N = 2 * CHUNK + 88  # records of the buffer before a record is inserted or replaced
BAD_AT = (0, CHUNK - 1, CHUNK, CHUNK + 1, BAD_N - 1)
BAD_RECORDS = {"corrupt_tag": b"\x09", "order": b"\x00\x02", "bad_enum": b"\x04" + struct.pack(">iqb", 1, 2, 9)}
CORRUPT5 = b"\x09\x01\x02\x03\x04"  # a corrupt tag that keeps the 5-byte grid


def bad_spans():
    """(name, bytes): a record that is not a BufferBuilt inserted before record k (what follows
    leaves the 5-byte grid, so many later threads see a bad record too: the lowest wins); records
    replaced by a corrupt tag of the same length at k1 < k2 in different chunks, in one chunk, and
    at a low k1 with one more in every later chunk."""
    out = []
    for j, (kind, rec) in enumerate(BAD_RECORDS.items()):
        base = good(BAD_N, 200 + j)
        for k in BAD_AT:
            out.append((f"{kind}_at_{k}", base[:5 * k] + rec + base[5 * k:]))
    for name, ks in (("two_chunks", (100, CHUNK + 144)), ("one_chunk", (3, 200)),
                     ("every_chunk", (3,) + tuple(CHUNK * c + 17 for c in range(1, 8)))):
        n = max(BAD_N, ks[-1] + 50)
        buf = bytearray(good(n, 210 + len(ks)))
        for k in ks:
            buf[5 * k:5 * k + 5] = CORRUPT5
        out.append((f"replaced_{name}", bytes(buf)))
    return out


def replaced_at(buf):
    """Records of a buffer on the 5-byte grid whose tag is not 07."""
    return [k for k in range(len(buf) // 5) if buf[5 * k] != 7]


# ---- many spans --------------------------------------------------------------------------------------------
SPAN_COUNTS = (CLASSIFY - 1, CLASSIFY, CLASSIFY + 1)
PER_PARTITION = 32  # subpartitions named per partition (the subpartition index is a byte)


def many_spans(ns):
    """ns spans of 3..7 records; the last one holds an Order after its second record, its
    neighbours are clean."""
    out = [good(3 + j % 5, 300 + j) for j in range(ns)]
    out[-1] = out[-1][:10] + b"\x00\x07" + out[-1][10:]
    return out


def sub_id(j):
    """(irp_lower, irp_upper, subpartition) of span j of a call."""
    return 1000 + j // PER_PARTITION, 2000 + j // PER_PARTITION, j % PER_PARTITION
