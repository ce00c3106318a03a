"""The scenes of test_gpu_bufsizes_edges.py hit what its docstring claims (no GPU, no engine; the
reference loop alone): sizes whose four bytes all take nonzero values and negatives, span lengths
either side of the 256-record chunk with every partial tail, a first bad record at every chunk
seam, and span counts either side of the classify kernel's 64."""
import os
import struct

import _bufsizes_scenes as S

E_TRUNCATED, E_CORRUPT_TAG, E_BAD_ENUM, E_NOT_BUFFER_BUILT = -3, -2, -4, -15


def test_constants_are_the_kernels():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clonos_amd", "csrc")
    kernels = open(os.path.join(csrc, "replay.hip")).read()
    assert "kBufThreads = 256;" in kernels and "(n_spans + 63) / 64), dim3(64)" in kernels
    assert "kRecPerChunk = 256;" in open(os.path.join(csrc, "engine_replay.cpp")).read()
    assert (S.CHUNK, S.CLASSIFY) == (256, 64)
    assert (S.R.E_NOT_BUFFER_BUILT, S.R.E_TRUNCATED, S.R.E_CORRUPT_TAG) == (E_NOT_BUFFER_BUILT, E_TRUNCATED, E_CORRUPT_TAG)


def test_values_cover_every_byte_and_the_sign():
    assert {S.INT32_MIN, -1, 0, 1, S.INT32_MAX, 0x01020304} <= set(S.VALUES)
    assert all(S.INT32_MIN <= v <= S.INT32_MAX for v in S.VALUES)
    vals = S.values(40, 1)
    assert vals[:len(S.VALUES)] == S.VALUES and len(set(vals)) > 30
    buf = S.bb(S.VALUES)
    for byte in range(1, 5):  # each of the four size bytes takes a nonzero value, alone as well
        col = {buf[5 * k + byte] for k in range(len(S.VALUES))}
        assert len(col - {0}) >= 3
        assert any(buf[5 * k + byte] and not any(buf[5 * k + b] for b in range(1, 5) if b != byte)
                   for k in range(len(S.VALUES)))
    assert len(set(struct.pack(">i", 0x01020304))) == 4
    assert sum(v < 0 for v in S.VALUES) >= 4 and struct.pack(">i", S.VALUES[6]) == b"\x80\0\0\0"
    sizes, st, off, tag = S.expected(buf)
    assert (sizes, st, off, tag) == (S.VALUES, 0, -1, -1)
    # every span the tests run starts with them
    assert S.good(S.CHUNK, 5)[:5 * len(S.VALUES)] == buf


def test_length_spans():
    spans = dict(S.length_spans())
    lens = sorted(len(b) for b in spans.values())
    want = [0, 1, 2, 3, 4, 5, 10, 35, 5 * 255, 5 * 256, 5 * 257, 5 * 512, 5 * 513 + 3] + [5 * 256 + r for r in range(1, 5)]
    assert set(lens) == set(want)
    for name, buf in spans.items():
        sizes, st, off, tag = S.expected(buf)
        assert len(sizes) == len(buf) // 5, name
        if len(buf) % 5 == 0:
            assert st == 0, name
            continue
        whole = len(buf) // 5 * 5
        assert off == whole and len(sizes) == whole // 5, name
        if "order" in name and len(buf) % 5 >= 2:  # an Order that decodes
            assert (st, tag) == (E_NOT_BUFFER_BUILT, 0), name
        else:
            assert (st, tag) == (E_TRUNCATED, buf[whole]), name
    # both kinds of tail at every length, alone and after an exact chunk
    for r in range(1, 5):
        for t in S.TAILS:
            assert len(spans[f"only_{t}_{r}"]) == r and len(spans[f"chunk_plus_{t}_{r}"]) == 5 * S.CHUNK + r
    # all of them as the subpartitions of one call: bases that are no multiple of anything
    bases, at = [], 0
    for buf in spans.values():
        bases.append(at)
        at += len(buf) // 5
    assert any(b % 2 for b in bases) and any(b % S.CHUNK not in (0, 1, 2, 3) for b in bases)


def test_first_bad_record_scenes():
    spans = dict(S.bad_spans())
    status = {"corrupt_tag": E_CORRUPT_TAG, "order": E_NOT_BUFFER_BUILT, "bad_enum": E_BAD_ENUM}
    assert S.BAD_AT == (0, 255, 256, 257, S.BAD_N - 1) and S.BAD_N > 2 * S.CHUNK
    for kind, st_want in status.items():
        for k in S.BAD_AT:
            sizes, st, off, tag = S.expected(spans[f"{kind}_at_{k}"])
            assert (len(sizes), st, off, tag) == (k, st_want, 5 * k, S.BAD_RECORDS[kind][0])
    two = spans["replaced_two_chunks"]
    ks = S.replaced_at(two)
    assert len(two) % 5 == 0 and len(ks) == 2 and ks[0] // S.CHUNK != ks[1] // S.CHUNK
    assert S.expected(two)[1:] == (E_CORRUPT_TAG, 5 * ks[0], 9) and len(S.expected(two)[0]) == ks[0]
    one = S.replaced_at(spans["replaced_one_chunk"])
    assert len(one) == 2 and one[0] // S.CHUNK == one[1] // S.CHUNK and one[0] // 64 != one[1] // 64
    every = S.replaced_at(spans["replaced_every_chunk"])
    assert [k // S.CHUNK for k in every] == list(range(8)) and every[0] == 3
    assert S.expected(spans["replaced_every_chunk"])[1:] == (E_CORRUPT_TAG, 15, 9)


def test_many_spans():
    assert S.SPAN_COUNTS == (63, 64, 65)
    for ns in S.SPAN_COUNTS:
        spans = S.many_spans(ns)
        assert len(spans) == ns
        res = [S.expected(b) for b in spans]
        assert [r[1] for r in res] == [0] * (ns - 1) + [E_NOT_BUFFER_BUILT]
        assert res[-1][2:] == (10, 0) and len(res[-1][0]) == 2
        assert all(3 <= len(r[0]) <= 7 for r in res[:-1])
        ids = [S.sub_id(j) for j in range(ns)]
        assert len(set(ids)) == ns and all(0 <= i[2] < 128 for i in ids) and len({i[0] for i in ids}) >= 2
    # the bad span of 64 is the first workgroup's last, that of 65 the second workgroup's first
    assert (64 - 1) // S.CLASSIFY == 0 and (65 - 1) // S.CLASSIFY == 1 and (65 - 1) % S.CLASSIFY == 0
