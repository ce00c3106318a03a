"""The decode edge scenes (_decode_scenes.py) cover what they claim, proved without a GPU: by
the restated tile plans every kind's record is split by a tile end at every byte, every
reachable halo-staging branch is reached by a tile with a record header across its end, and
the CPU oracle shows that a decode that read past a span's end, or that got a tile's halo
wrong, would return something else than the right answer."""
import numpy as np
import pytest

import _decode_scenes as S
import _oracle as O


@pytest.fixture(scope="module")
def fam():
    return {"A": S.family_a(), "A_thin": S.family_a_thin(), "B": S.family_b(), "C": S.family_c(), "E": S.family_e()}


def _splits(sc, T):
    """k for every tile end inside or at the ends of the scene's record: the tile end lies k
    bytes after the record's start."""
    L = len(sc.span) - sc.at  # upper bound; the caller filters by the kind's length
    return [t.span_off + t.len - sc.at for t in S.host_tiles(sc.residue, len(sc.span), T)
            if 0 <= t.span_off + t.len - sc.at <= L]


def test_kind_table():
    L = {k.name: len(k.rec) for k in S.KINDS}
    assert (L["order"], L["timestamp"], L["rng"], L["buffer_built"], L["ignore_cp"], L["timer_plain"],
            L["source_noref"], L["ser_null"]) == (2, 9, 5, 5, 13, 14, 23, 6)
    for n in (0, 1):
        assert (L[f"timer_name_n{n}"], L[f"source_ref_n{n}"], L[f"ser_string_n{n}"]) == (18 + n, 27 + n, 8 + n)
    for stem in ("timer_name", "source_ref", "ser_string"):
        assert {L[f"{stem}_L{x}"] for x in S.LONG_LENGTHS} == set(S.LONG_LENGTHS)
    # the thresholds the lengths straddle
    assert {S.LM_MAX - 1, S.LM_MAX, S.LM_MAX + 1, S.SPEC_MAX - 1, S.SPEC_MAX, S.SPEC_MAX + 1} <= set(S.LONG_LENGTHS)
    assert max(S.LONG_LENGTHS) > S.CANON_REACH
    for k in S.KINDS:  # every record alone is what the oracle calls one record of that length
        st, r, _, _ = O.decode(k.rec)
        assert st == 0 and len(r["tag"]) == 1 and r["tag"][0] == k.rec[0], k.name
        # distinct nonzero bytes in the fixed fields (a stream's header is the format's own)
        h = k.rec[1:min(k.hdr, 13)]
        assert S.is_ser(k) or (0 not in h and len(set(h)) == len(h)), k.name


def test_split_coverage_aligned(fam):
    """Residue 0: for every kind, each T and every k of split_points, some family-A scene has
    a tile end exactly k bytes after the record's start."""
    got = {}
    for sc in fam["A"]:
        got.setdefault((sc.kind, sc.T), set()).update(_splits(sc, sc.T))
    for k in S.KINDS:
        for T in S.TILES:
            assert set(S.split_points(k)) <= got[k.name, T], (k.name, T, sorted(set(S.split_points(k)) - got[k.name, T]))


def test_split_coverage_residues(fam):
    """The thinned variant at its own density.  It holds a quarter of family A's starts and a
    residue gets a fifteenth of those; family A splits about 800 header bytes per T (39 kinds,
    about 20 header bytes each), so a residue sees about 13.  Asserted: at each T and residue
    1..15 at least 6 different header bytes 1..26 are split and each tag with a long header
    (Serializable, TimerTrigger, SourceCheckpoint) has a header split; every header byte 1..26 is
    split at 3 residues or more; every kind meets a quarter of its split points over the residues."""
    by_res, by_kind, by_k = {}, {}, {}
    for sc in fam["A_thin"]:
        assert 1 <= sc.residue <= 15
        kind = S.KIND[sc.kind]
        ks = [k for k in _splits(sc, sc.T) if k <= len(kind.rec)]
        by_kind.setdefault((sc.kind, sc.T), set()).update(ks)
        for k in ks:
            if 0 < k < min(len(kind.rec), 27):
                by_res.setdefault((sc.T, sc.residue), []).append((k, kind.rec[0]))
                by_k.setdefault((sc.T, k), set()).add(sc.residue)
    for T in S.TILES:
        for r in range(1, 16):
            assert len({k for k, _ in by_res[T, r]}) >= 6, (T, r)
            assert {3, 4, 5} <= {tag for _, tag in by_res[T, r]}, (T, r)
        for k in range(1, 27):
            assert len(by_k[T, k]) >= 3, (T, k, by_k[T, k])
    for k in S.KINDS:
        for T in S.TILES:
            want = set(S.split_points(k))
            assert 4 * len(by_kind[k.name, T] & want) >= len(want) - 3, (k.name, T)


# A branch of stage_finish no engine configuration reaches, with the reason; every other branch
# must be reached by a tile with a record header across its end.
UNREACHABLE = {
    "far_bytes": "a tile that has a next tile in its span ends on a 16-byte boundary of its buffer (a host span's "
                 "first tile ends at T - delta + delta, a log's tiles are cut at multiples of 16) and the next "
                 "tile's delta is 0, so (hi - n1.delta) & 15 is always 0",
    "next_long": "phase 3, the only caller with a halo above 64, always passes the next tile's descriptor, so a "
                 "next tile that holds the halo is taken by far16 before",
}


def _header_across(tile_end, rec_starts, rec_len):
    """Some record's first 27 bytes (the longest header) lie across span offset tile_end."""
    return any(s < tile_end < s + min(rec_len, 27) for s in rec_starts)


def test_staging_branch_coverage(fam):
    reached = {}

    def visit(tiles, span_len, rec_starts, rec_len, what):
        for i, t in enumerate(tiles):
            if not _header_across(t.span_off + t.len, rec_starts, rec_len):
                continue
            for name, H, has_n1 in S.CALLERS:
                reached.setdefault((name, S.stage_branch(tiles, i, span_len, H, has_n1)), what)

    for f in ("A", "A_thin", "B", "E"):
        for sc in fam[f]:
            if sc.T != S.T_FUSED:
                continue
            L = len((S.KIND.get(sc.kind) or S.B_KIND.get(sc.kind) or S.Kind("", b"x" * 27, 27)).rec)
            visit(S.host_tiles(sc.residue, len(sc.span), S.T_FUSED), len(sc.span), [sc.at], L, f)
    for C in S.SEGMENTS:
        for lg in S.d_logs(C)[::7 if C == 16384 else 1]:
            L, p, n = len(S.KIND[lg.kind].rec), len(lg.prefix), len(lg.prefix) + len(lg.body)
            visit(S.log_tiles(0, n, C, S.T_FUSED), n, lg.starts, L, f"D{C}")
            visit(S.log_tiles(p, n - p, C, S.T_FUSED), n - p, [s - p for s in lg.starts], L, f"D{C}+prefix")
    got = {b for _, b in reached}
    # ("none": a span's last tile, no halo, so no header across its end)
    assert got == set(S.BRANCHES) - set(UNREACHABLE) - {"none"}, (sorted(got), reached)
    # by caller: the 64-byte halo's two ways with a next tile, the walk without one, phase 3's
    for key in (("count_emit_small", "near"), ("count_emit_small", "walk"), ("chunk_exit", "walk"),
                ("phase3", "far16"), ("phase3", "walk")):
        assert key in reached, key
    # the walk with a next tile at hand needs a next tile shorter than the halo: small segments
    assert reached["count_emit_small", "walk"].startswith("D") and reached["phase3", "walk"].startswith("D")
    # short last tiles: the last tile is r bytes, every r of B_R; below 64 the halo is r bytes and the zero pad follows
    halos = set()
    for sc in fam["B"]:
        t = S.host_tiles(0, len(sc.span), S.T_FUSED)
        assert len(t) == 2 and S.stage_branch(t, 0, len(sc.span), S.HALO, True) == "near"
        halos.add(t[1].len)
    assert halos == set(S.B_R)


def test_unreachable_branches_are_unreachable():
    """The reason given for far_bytes, checked over the plans: every tile with a successor in
    its span ends 16-byte aligned and the successor's delta is 0."""
    plans = [S.host_tiles(d, n, T) for d in range(16) for n in (1, 100, 8191, 8192, 8193, 40000) for T in S.TILES]
    plans += [S.log_tiles(st, n, C, T) for C in S.SEGMENTS + (4096, 65536) for st in (0, 1, 15, 16, 47, 8191)
              for n in (1, 63, 64, 65, 9000, 40000) for T in S.TILES]
    for tiles in plans:
        for a, b in zip(tiles, tiles[1:]):
            assert (a.delta + a.len) % 16 == 0 and b.delta == 0 and b.span_off == a.span_off + a.len


def test_good_scenes_decode_cleanly(fam):
    for f in ("A", "A_thin", "B", "E"):
        for sc in fam[f]:
            st, r, _, _ = O.decode(sc.span)
            assert st == 0 and sc.at in r["off"], (f, sc.kind, sc.T, sc.at, sc.note)
    for C in S.SEGMENTS:
        for lg in S.d_logs(C)[::5 if C == 16384 else 1]:
            assert len(lg.prefix) % 16 != 0 and len(lg.prefix) + len(lg.body) < 65536
            st, r, _, _ = O.decode(lg.prefix + lg.body)
            assert st == 0 and set(lg.starts) <= set(r["off"].tolist()), (C, lg.kind)
            st, r, _, _ = O.decode(lg.body)
            assert st == 0 and {s - len(lg.prefix) for s in lg.starts} <= set(r["off"].tolist()), (C, lg.kind)


def test_log_starts_cover_every_residue():
    for C in S.SEGMENTS[:-1]:
        m, got = min(C, 64), {}
        for lg in S.d_logs(C):
            got.setdefault(lg.kind, set()).update(s % m for s in lg.starts)
        for k in S.KINDS:
            assert got[k.name] == set(range(m)), (C, k.name)
    big = S.d_big_logs()
    got = {}
    for lg in big:
        got.setdefault(lg.kind, set()).update(lg.starts)
    for k in S.KINDS:
        for T in S.TILES:  # physical offsets 8192 and 16384
            assert {T - x for x in S.split_points(k)} <= got[k.name], (k.name, T)


def _same(a, b):
    return a[0] == b[0] and a[2] == b[2] and all(np.array_equal(a[1][f], b[1][f]) for f in a[1])


def test_truncations_would_show_an_overread(fam):
    """Family C: the span alone is an error at the expected offset, the record's start.  A cut
    record: with the gap's bytes behind the span the oracle returns something else -- the
    record whole and more records, no error -- so a decode that read past the span's end
    would differ.  (An invalid record is invalid whatever follows it: its scenes pin the error
    fields where the bytes that decide them lie across a tile end.)"""
    for sc in fam["C"]:
        alone = O.decode(sc.span)
        assert alone[0] != 0 and alone[2] == sc.at, (sc.kind, sc.note, alone[0], alone[2])
        if sc.note.startswith("cut"):
            over = O.decode(sc.span + sc.gap)
            assert not _same(alone, over), (sc.kind, sc.note)
            assert over[0] == 0 and len(over[1]["tag"]) > len(alone[1]["tag"]) + 1, (sc.kind, sc.note)


def test_bad_halo_would_show(fam):
    """Families A and B: with the 64 bytes behind the tile end that the record crosses zeroed
    (what a tile's image holds when its halo was not staged: the zero pad), the oracle's
    result changes or becomes an error.  This holds where the tile end lies in the record's
    header or the halo reaches the next record; a tile end deeper in a payload leaves only
    payload bytes in the halo, which no decoded field holds."""
    n = 0
    for f in ("A", "A_thin", "B"):
        for sc in fam[f]:
            kind = S.KIND.get(sc.kind) or S.B_KIND[sc.kind]
            L = len(kind.rec)
            for t in S.host_tiles(sc.residue, len(sc.span), sc.T)[:-1]:
                e = t.span_off + t.len
                if not sc.at < e < sc.at + L:  # the record does not cross this tile end
                    continue
                if e - sc.at >= kind.hdr and min(e + S.HALO, len(sc.span)) <= sc.at + L:
                    continue  # only payload bytes behind it
                z = bytearray(sc.span)
                z[e:e + S.HALO] = bytes(len(z[e:e + S.HALO]))
                if bytes(z) == sc.span:  # SourceCheckpoint's hasRef = 0 alone behind the tile end
                    assert sc.kind == "source_noref" and e == sc.at + 22
                    continue
                assert not _same(O.decode(sc.span), O.decode(bytes(z))), (f, sc.kind, sc.T, sc.at, sc.note)
                n += 1
    assert n >= 1500  # the check met that many crossings


def test_batch_limits(fam):
    groups = {f: S.by_group(fam[f], {**S.KIND, **S.B_KIND}) for f in ("A", "A_thin", "B", "E")}
    groups["C"] = S.by_group([sc for sc in fam["C"] if " mid" in sc.note])
    for f, gs in groups.items():
        small = large = 0
        for g, scenes in gs.items():
            for T in S.TILES:
                for b in S.batches([sc for sc in scenes if sc.T == T]):
                    blob, spans = S.batch(b)
                    nt = S.n_tiles(b)
                    assert len(blob) <= S.SMALL_BYTES and len(b) <= S.SMALL_SPANS and nt <= S.SMALL_TILES, (f, g)
                    for (o, _), sc in zip(spans, b):
                        assert o % 16 == (sc.residue if o else 0)
                    small += len(b) <= S.ARG_SPANS and nt <= S.ARG_TILES
                    large += len(b) > S.ARG_SPANS or nt > S.ARG_TILES
        assert small and large, (f, small, large)
    for C in S.SEGMENTS:
        logs = S.d_logs(C)
        small = large = 0
        for lo, hi in S.d_batches(logs):
            n = sum(len(l.prefix) + len(l.body) for l in logs[lo:hi])
            nt = sum(len(S.log_tiles(0, len(l.prefix) + len(l.body), C, S.T_FUSED)) for l in logs[lo:hi])
            assert n <= S.SMALL_BYTES and hi - lo <= S.SMALL_SPANS
            small += hi - lo <= S.ARG_SPANS and nt <= S.ARG_TILES
            large += hi - lo > S.ARG_SPANS or nt > S.ARG_TILES
        assert large and (small or C < 16384), (C, small, large)
