"""The scenes of test_gpu_copy_edges.py cover what its docstring claims (no GPU, no engine):
every (source residue, destination residue, length) triple of the short gather and scatter
sweeps, both trip counts of copy_range's loop in the gather and in the scatter, every
remainder of the piece count mod 8, and the segment-edge cases."""
import itertools

import _copy_scenes as S


def test_data_avoids_the_sentinels():
    b = S.data(100000, 1)
    assert min(b) == 1 and max(b) == 254
    assert S.FILL == 0xFF


def test_chunk_and_piece_arithmetic():
    assert S.chunks(0, 16) == 1 and S.chunks(15, 2) == 2 and S.chunks(1, 15) == 1 and S.chunks(5, 0) == 0
    assert S.chunks(16, 16384) == 1024 and S.chunks(17, 16384) == 1025
    assert S.trips(1024, 256) == 1 and S.trips(1025, 256) == 2 and S.trips(256, 64) == 1 and S.trips(257, 64) == 2
    assert S.pieces(60, 10, 64, 7) == [(60, 7, 4), (64, 11, 6)]
    assert S.pieces(64, 128, 64, 0) == [(64, 0, 64), (128, 64, 64)]
    pos, size = S.place([(5, 0), (3, 15), (1, 15), (16, 1)])
    assert pos == [0, 31, 63, 65] and size == 112
    buf = S.source_buffer([b"\x01" * 5, b"\x02" * 3], pos[:2], size)
    assert buf[:5].tolist() == [1] * 5 and buf[5:31].tolist() == [255] * 26 and buf[31:34].tolist() == [2] * 3
    want = S.packed([b"ab", b"c"], 3)
    assert len(want) == S.buffer_size(3) and want[19:22] == b"abc" and set(want[:19] + want[22:]) == {0xFF}
    assert len(want) - 22 >= S.SLACK


def test_epochs_end_on_every_residue():
    starts = S.epoch_starts()
    assert len(S.EPOCH_LENS) == 16
    for t in range(16):
        assert (starts[t] + S.EPOCH_LENS[t]) % 16 == t
        assert max(S.SHORT_L) <= S.EPOCH_LENS[t]
        for L in S.SHORT_L:
            assert S.short_range(t, L)[0] % 16 == (t - L) % 16


def test_packed_gather_has_every_triple():
    reqs = S.short_requests()
    assert len(reqs) == 16 * len(S.SHORT_L) == len(set(reqs))
    got = set()
    for d in range(16):
        got |= S.short_triples(reqs, d)
    assert got == set(itertools.product(range(16), range(16), S.SHORT_L))
    # ranges that cross a 64-byte segment, and ranges inside one
    n_pieces = {len(S.pieces(*S.short_range(t, L), 64, 0)) for t, L in reqs}
    assert n_pieces == {1, 2, 3}


def test_isolated_gather_has_every_triple():
    cases = S.isolated_cases()
    got = {(S.short_range(t, L)[0] % 16, d, L) for t, d, L in cases}
    assert got == set(itertools.product(range(16), range(16), S.ISO_L))
    assert all(d + L + S.SLACK <= S.ISO_SLOT for _, d, L in cases)  # slack inside the slot
    want = S.isolated_expect(S.short_log(), cases)
    assert len(want) == len(cases) * S.ISO_SLOT + S.SLACK
    t, d, L = cases[100]
    p, n = S.short_range(t, L)
    assert want[100 * S.ISO_SLOT + d:100 * S.ISO_SLOT + d + n] == S.short_log()[p:p + n]


def test_piece_counts_have_every_remainder():
    batches = S.count_batches()
    singles = [b for b in batches if len(b) == 1]
    assert [S.count_pieces(b) for b in singles] == list(range(1, 26))
    multi = [S.count_pieces(b) for b in batches if len(b) > 1]
    assert sorted(n % 8 for n in multi) == list(range(8)) and all(n > 8 for n in multi)
    assert {S.count_pieces(b) % 8 for b in singles} == set(range(8))
    assert all(n <= S.COUNT_N for b in batches for n in b)


def test_gather_trips():
    """Whole-segment pieces at 1024 chunks (one trip) and 1025 (a second trip of one chunk); a
    first piece of 16383 bytes at both counts.  A first piece of 16369 bytes fills 1024 chunks
    at every destination residue (residue + 16369 <= 16384): one trip, never two."""
    seen = {}
    for d in S.TRIP_BASES:
        for n, r, c in S.trip_pieces(d):
            seen.setdefault(n, set()).add((r, c))
    assert {c for _, c in seen[16384]} == {1024, 1025}
    assert {c for _, c in seen[16383]} == {1024, 1025}
    assert {c for _, c in seen[16369]} == {1024} and len(seen[16369]) == len(S.TRIP_BASES)
    assert {S.trips(c, 256) for v in seen.values() for _, c in v} == {1, 2}
    assert (0, 1024) in seen[16384] and any(r and c == 1025 for r, c in seen[16384])
    # the one-byte first piece (offset 16383), the log's last five bytes, the piece from offset 16
    assert set(seen) == {1, 5, 16368, 16369, 16383, 16384}


def test_scatter_trips():
    cases = S.trip_scatter_cases()
    assert len(cases) == 90
    counts = set()
    for w, s, L in cases:
        for p, k, c in S.scatter_chunks(w, L, S.BIG_SEG):
            assert p % S.BIG_SEG + k <= S.BIG_SEG
            counts.add(c)
    # one trip of a wave is 256 chunks: the last chunk of one and of two trips, the first of the
    # next, and a whole segment (1024 chunks, four trips: a chunk never crosses a segment)
    assert {256, 257, 512, 513, 1024} <= counts and max(counts) == 1024
    assert {S.trips(c, 64) for c in counts} == {1, 2, 3, 4}
    assert {(w, s) for w, s, _ in cases} == set(itertools.product(S.TRIP_RES, S.TRIP_RES))


def test_short_scatter_has_every_triple_and_the_segment_edges():
    cases = S.scatter_cases()
    assert set(cases) == set(itertools.product(range(16), range(16), S.SCATTER_L)) and len(cases) == 3584
    assert any(S.ends_on_segment_end(w, L) for w, _, L in cases)
    assert {(w, L) for w, _, L in cases if S.ends_on_segment_end(w, L)} == {(0, 64), (1, 63), (15, 49)}
    assert any(S.starts_on_segment_start(w, L) and w == 0 for w, _, L in cases)
    assert any(S.starts_on_segment_start(w, L) and w != 0 for w, _, L in cases)
    pos, size = S.place([(L, s) for _, s, L in cases])
    assert all(p % 16 == s for p, (_, s, _) in zip(pos, cases))
    assert all(a + c[2] <= b for a, b, c in zip(pos, pos[1:], cases)) and pos[-1] + cases[-1][2] + 16 <= size


def test_staged_appends_have_every_shift():
    cases = S.staged_cases()
    shifts = S.staged_shifts(cases)
    assert 200 <= len(cases) <= 500
    assert set(shifts) == set(range(16))
    assert {L for _, L in cases} == set(S.SCATTER_L) and {w for w, _ in cases} == set(range(16))
    # every shift at a length of a single edge chunk and at one with whole chunks
    assert {(sh, L > 32) for sh, (_, L) in zip(shifts, cases)} == set(itertools.product(range(16), (False, True)))


def test_inflight_buffers_have_every_source_residue():
    for seg in (64, S.BIG_SEG):
        cases = S.ifl_cases(seg)
        ls = S.SCATTER_L + ([16384, 16385] if seg == S.BIG_SEG else [])
        assert set(cases) == set(itertools.product(ls, range(16)))
        # replayed back to back at each base: many destination residues per length
        for b in S.IFL_BASES:
            off, res = 0, set()
            for L, _ in cases:
                res.add((b + off) % 16)
                off += L
            assert len(res) == 16
