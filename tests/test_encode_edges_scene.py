"""The scenes of test_gpu_encode_edges.py hit what its docstring claims (no GPU, no engine; the
oracle alone): every (kind, slot of a thread) and (kind, side of a seam) pair, block totals of
28 671, 28 672 and 28 673 bytes from the oracle's record lengths, the blocks that hold the wide
rows of the scan-round scene, and the lowest bad record of every validation scene."""
import itertools

import numpy as np

import _encode_scenes as S
import _oracle as O


def oracle_lens(soa):
    """Every record's length as orc_encode gives it, one record at a time."""
    return np.array([len(O.encode_soa(*S.cut(soa, i, i + 1))) for i in range(len(soa[0]))], np.int64)


def block_totals(lens):
    return [int(lens[a:a + S.BLOCK].sum()) for a in range(0, len(lens), S.BLOCK)]


def test_constants_are_the_kernels():
    src = open(O.ROOT + "/clonos_amd/csrc/encode.hip").read()
    assert "kEncThreads = 256;" in src and "kEncPer = 4;" in src and "kEncLds = 28 * 1024;" in src
    assert "b0 += 1024" in src and "blk <= kEncLds" in src
    assert (S.BLOCK, S.PER, S.WAVE, S.STAGE, S.SCAN) == (1024, 4, 256, 28672, 1024)


def test_payload_bytes_avoid_the_sentinels():
    b = S.payload(np.random.default_rng(1), 100000)
    assert min(b) == 1 and max(b) == 254 and S.FILL == 0xFF


def test_record_lengths_are_the_oracles():
    soa = S.extremes()
    np.testing.assert_array_equal(S.lens_of(soa), oracle_lens(soa))
    soa = S.range_batch()
    np.testing.assert_array_equal(S.lens_of(soa), oracle_lens(soa))
    assert len(O.encode_soa(*soa)) == int(S.lens_of(soa).sum())


def test_lengths_and_mixes():
    scenes = S.length_scenes()
    assert {(m, n) for m, n, _ in scenes} == set(itertools.product(S.MIXES, S.LENGTHS))
    assert S.LENGTHS == [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
    for mix, n, soa in scenes:
        tag = soa[0]
        assert len(tag) == n
        if mix == "narrow":
            assert len(soa[2]) == 0 and (n < 64 or set(tag.tolist()) == {0, 1, 2, 7})
        elif mix == "wide":
            assert len(soa[2]) == n and set(tag.tolist()) == {S.TAG[S.mix_kinds(mix, n, S.LENGTHS.index(n))[0]]}
        else:
            assert n < 13 or set(tag.tolist()) == set(range(8))
    # every wide kind is the one kind of some batch
    assert {S.mix_kinds("wide", n, j)[0] for j, n in enumerate(S.LENGTHS)} == set(S.WIDE)
    assert np.gcd(len(S.KINDS), S.PER) == 1


def test_every_kind_at_every_slot_and_seam():
    slots, seams = set(), set()
    for kind, side, soa in S.place_scenes():
        kinds = S.place_kinds(kind, side)
        assert len(soa[0]) == S.PLACE_N and [S.TAG[k] for k in kinds] == soa[0].tolist()
        sl, se = S.place_coverage(kinds)
        slots |= {x for x in sl if x[0] == kind}
        seams |= {x for x in se if x[0] == kind}
    assert slots == set(itertools.product(S.KINDS, range(S.PER)))
    assert seams == set(itertools.product(S.KINDS, S.SEAMS, (0, 1)))
    assert S.SEAMS == {"wave": (255, 256), "block": (1023, 1024), "block2": (2047, 2048)}
    # the variants are what their names say
    for kind, side, soa in S.place_scenes():
        if kind in S.NARROW:
            continue
        k = int(np.flatnonzero(soa[2] == S.SEAMS["wave"][side])[0])
        sub, ln = int(soa[7][k]), int(soa[6][k])
        assert S.has_payload(S.TAG[kind], sub) == (kind not in ("ignore", "timer_other", "source_plain"))
        assert (ln > 0) == (kind in ("timer6_name", "source_ref", "serial"))
        assert kind != "timer_other" or sub < 6


def test_wide_prefix_scenes():
    sc = dict(S.prefix_scenes())
    full = sc["full_block"]
    assert (full[2][:S.BLOCK] == np.arange(S.BLOCK)).all() and set(full[0][:S.BLOCK].tolist()) == {3, 4, 5, 6}
    gaps = sc["empty_blocks"]
    assert gaps[2].tolist() == [S.BLOCK - 1, 3 * S.BLOCK, 4 * S.BLOCK - 1, 4 * S.BLOCK]
    assert S.wide_blocks(gaps) == [0, 3, 4] and len(gaps[0]) > 5 * S.BLOCK
    last = sc["last"]
    assert last[2].tolist() == [len(last[0]) - 1] and len(last[0]) > S.BLOCK


def test_extremes_cover_every_field():
    tag, v0, w_idx, w_rc, w_v1, _, w_len, w_sub, _ = S.extremes()
    i64 = {x for x in S.I64}
    for t, vals in ((0, S.I8 + S.ABOVE8), (2, S.I32 + S.ABOVE32), (7, S.I32 + S.ABOVE32), (1, S.I64)):
        assert set(v0[tag == t].tolist()) == set(vals)
    assert not any(-(1 << 7) <= v < 1 << 7 for v in S.ABOVE8) and not any(-(1 << 31) <= v < 1 << 31 for v in S.ABOVE32)
    wt = tag[w_idx]
    for t in (4, 5, 6):
        m = wt == t
        assert i64 <= set(v0[w_idx[m]].tolist()) and set(S.I32) <= set(w_rc[m].tolist())
    assert i64 <= set(w_v1[wt == 5].tolist())
    assert set(w_sub[wt == 4].tolist()) == set(S.TIMER_SUBS) == set(range(7))
    assert set(w_sub[wt == 5].tolist()) == set(S.SOURCE_SUBS) == {0, 1, 0x80, 0x81}
    for t, sub in ((4, 6), (5, 0x80), (5, 0x81), (3, 0)):  # a payload row with and without bytes
        m = (wt == t) & (w_sub == sub)
        assert (w_len[m] == 0).any() and (w_len[m] > 0).any()


def test_stage_limit_block_totals():
    seen = {}
    for name, soa, totals in S.stage_scenes():
        lens = oracle_lens(soa) if name.startswith(("staged", "names")) else S.lens_of(soa)
        assert block_totals(lens) == totals, name
        assert len(O.encode_soa(*S.cut(soa, 0, S.BLOCK))) == totals[0], name  # the first block, by the oracle
        seen[name] = totals
    for t in (S.STAGE - 1, S.STAGE, S.STAGE + 1):
        assert {f"mid_{t}", f"first_{t}", f"last_{t}"} <= set(seen)
    assert (S.STAGE - 1, S.STAGE, S.STAGE + 1) == (28671, 28672, 28673)
    assert seen["staged_direct_one"] == [28672, 28673, 23]
    assert seen["names_28672"][0] == 28672 and seen["names_28673"][0] == 28673
    for name, soa, _ in S.stage_scenes():
        if name.startswith("names"):  # the limit through many medium payloads: no record is long
            assert int(S.lens_of(soa).max()) < 64
        elif not name.startswith("staged"):
            at = {"mid": 500, "first": 0, "last": S.BLOCK - 1}[name.split("_")[0]]
            assert soa[2].tolist() == [at]


def test_scan_round_scene():
    soa = S.scan_round()
    n = len(soa[0])
    assert n == S.SCAN_N == 1026 * 1024 + 1
    assert (n + S.BLOCK - 1) // S.BLOCK == S.SCAN_BLOCKS == 1027 > S.SCAN  # a second round, of three blocks
    assert S.wide_blocks(soa) == [0, 1023, 1024, 1025, 1026]
    assert (np.diff(soa[2].astype(np.int64)) > 0).all() and soa[2][-1] == n - 1
    assert set(soa[0][soa[2]].tolist()) == {4, 5, 6} and not soa[6].any()
    assert not any(S.has_payload(int(t), int(s)) for t, s in zip(soa[0][soa[2]], soa[7]))
    narrow = np.ones(n, bool)
    narrow[soa[2]] = False
    assert set(soa[0][narrow].tolist()) == {0, 1, 2, 7}
    assert S.first_bad(soa) is None


def test_validation_scenes_expect_the_lowest_bad_record():
    base = S.valid_batch()
    n, nw = len(base[0]), len(base[2])
    assert S.first_bad(base) is None and n == 2 * S.BLOCK + 2
    want = {f"tag{b}_at_{p}": p for b in (8, 255) for p in (0, S.BLOCK - 1, S.BLOCK, n - 1)}
    want.update(two_blocks=300, one_thread=40, one_row_too_many=n, one_row_too_few=int(base[2][-1]))
    in_block = [int(i) for i in base[2] if S.BLOCK <= i < 2 * S.BLOCK]
    want.update(row_names_another_first=in_block[0], row_names_another_last=in_block[-1])
    got = {name: bad for name, _, bad in S.validation_scenes()}
    p = got.pop("after_wide_in_thread")
    assert got == want
    assert int(base[0][p - 1]) in (3, 4, 5, 6) and (p - 1) // S.PER == p // S.PER
    for name, soa, bad in S.validation_scenes():
        assert len(soa[0]) == n and abs(len(soa[2]) - nw) <= 1
        if name == "one_thread":
            assert 40 // S.PER == 42 // S.PER and soa[0][42] == 8
        if name == "two_blocks":
            assert soa[0][1500] == 8 and 1500 // S.BLOCK != 300 // S.BLOCK


def test_payload_range_scenes():
    sc = {name: (soa, bad, ok) for name, soa, bad, ok in S.range_scenes()}
    base = S.range_batch()
    n_var = len(base[8])
    ends = base[5].astype(np.int64) + base[6]
    assert int(ends.max()) == n_var and S.first_bad(base) is None
    for name, over in (("over_by_1", 1), ("over_by_8", 8)):
        soa, bad, _ = sc[name]
        e = soa[5].astype(np.int64) + soa[6]
        assert int(e.max()) == n_var + over and (e > n_var).sum() == 1 and S.first_bad(soa) == bad == 7
    soa, bad, _ = sc["empty_past_the_end"]
    k = int(np.flatnonzero(soa[2] == bad)[0])
    assert (int(soa[5][k]), int(soa[6][k])) == (n_var + 1, 0) and S.first_bad(soa) == bad == 8
    soa, bad, ok = sc["wild_without_payload"]
    assert bad is None and S.first_bad(soa) is None and (soa[5] == 0xFFFFFFF0).sum() == 3
    assert sc["exact"][1] is None
