"""GPU: clonos_amd.replay.locate_divergence -- where a regenerated main log leaves its
recovered copy: the byte (clg_diff_logs), the epoch, the record and both determinants.

The oracle is os.path.commonprefix over the two byte strings and the CPU oracle's decode
(_oracle.decode) of each, combined by the record rule: k_side = the side's decoded records with
off <= offset, record = max(k_log, k_rec) - 1, a side's determinant its record at that index
when it has one.
"""
import os

import _oracle as O
import numpy as np
import pytest

from clonos_amd import CausalLogID, DecodedBatch, Engine
from clonos_amd import determinants as D
from clonos_amd import synth
from clonos_amd.replay import Divergence, locate_divergence, verify_replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recovered():
    """Three epochs of 120 encoded determinants, as a recovered response would carry them."""
    rng = np.random.default_rng(71)
    return [[D.encode(synth.random_determinant(rng)) for _ in range(120)] for _ in range(3)]


def oracle_side(b: bytes):
    """(record offsets, index -> Determinant) of the CPU oracle's decode of b (the records before
    the one at which it stops, if it stops)."""
    _, r, _, _ = O.decode(b)
    n = len(r["off"])
    batch = DecodedBatch(r["off"], r["tag"], r["v0"], r["w_idx"], r["w_rc"], r["w_v1"], r["w_var_off"],
                         r["w_var_len"], r["w_sub"], np.array([0, n], np.uint64), [np.frombuffer(b, np.uint8)])
    return [int(o) for o in r["off"]], lambda k: batch.determinant_at(0, k)


def expect(log_bytes: bytes, rec_bytes: bytes, epoch_starts):
    """The Divergence the record rule gives for the two byte strings (None: equal)."""
    if log_bytes == rec_bytes:
        return None
    off = len(os.path.commonprefix([log_bytes, rec_bytes]))
    kind = ("differs" if off < min(len(log_bytes), len(rec_bytes)) else
            "log_is_prefix" if len(log_bytes) < len(rec_bytes) else "recovered_is_prefix")
    ol, dl = oracle_side(log_bytes)
    orr, dr = oracle_side(rec_bytes)
    kl, kr = sum(o <= off for o in ol), sum(o <= off for o in orr)
    rec = max(kl, kr) - 1
    ep = max(e for e, s in enumerate(epoch_starts) if s <= off)
    if rec < 0:
        return Divergence(off, kind, ep, off - epoch_starts[ep], None, None, None, None)
    return Divergence(off, kind, ep, off - epoch_starts[ep], rec, ol[rec] if rec < len(ol) else orr[rec],
                      dl(rec) if rec < len(ol) else None, dr(rec) if rec < len(orr) else None)


def fill(eng, vertex, epochs_bytes):
    log = eng.open_log(CausalLogID.main(vertex))
    for ep, b in enumerate(epochs_bytes):
        log.appendDeterminant(b, ep)
    return log


def starts_of(epochs_bytes):
    return [0] + [int(x) for x in np.cumsum([len(b) for b in epochs_bytes])[:-1]]


@pytest.fixture(scope="module")
def located(recovered):
    """One engine with every regenerated log, and locate_divergence over all of them in one call."""
    whole = b"".join(b"".join(e) for e in recovered)
    flat = [r for e in recovered for r in e]
    with Engine(segment_bytes=256, pool_segments=4096) as eng:
        cases = {}

        def case(name, vertex, enc):
            eps = [b"".join(enc[120 * ep:120 * ep + 120 if ep < 2 else None]) for ep in range(3)]
            cases[name] = (fill(eng, vertex, eps), b"".join(eps), starts_of(eps))

        # the replay re-appended exactly the recovered records
        case("same", 1, list(flat))
        # two records of one length swapped in epoch 1
        i = next(k for k in range(120, 239) if len(flat[k]) == len(flat[k + 1]) and flat[k] != flat[k + 1])
        sw = list(flat)
        sw[i], sw[i + 1] = sw[i + 1], sw[i]
        case("swapped", 2, sw)
        # one Timestamp's value changed in its last byte
        t = next(k for k in range(240, 360) if flat[k][0] == D.TIMESTAMP)
        ts = list(flat)
        ts[t] = ts[t][:-1] + bytes([ts[t][-1] ^ 0x04])
        case("timestamp", 3, ts)
        # the regenerated log cut after a whole record, and in the middle of one (of 9 bytes or
        # more, cut in half: the log's decode stops at it)
        case("cut_whole", 4, flat[:300])
        m = next(k for k in range(130, 360) if len(flat[k]) >= 9)
        case("cut_mid", 5, flat[:m] + [flat[m][:len(flat[m]) // 2]])
        # the regenerated log went on after the recovered one ended
        case("longer", 6, flat + [D.encode(D.OrderDeterminant(3)), D.encode(D.TimestampDeterminant(77))])

        names = list(cases)
        items = [(cases[n][0].handle, 0, whole) for n in names]
        got = dict(zip(names, locate_divergence(eng, items)))
        want = {n: expect(cases[n][1], whole, cases[n][2]) for n in names}
        yield dict(eng=eng, whole=whole, flat=flat, cases=cases, names=names, items=items, got=got, want=want,
                   swapped=i, timestamp=t, cut=m)


def test_every_case_follows_the_record_rule(located):
    for n in located["names"]:
        assert located["got"][n] == located["want"][n], n


def test_reappended_log_is_equal(located):
    assert located["got"]["same"] is None


def test_swapped_records(located):
    flat, i, d = located["flat"], located["swapped"], located["got"]["swapped"]
    assert d.kind == "differs" and d.epoch == 1 and d.record == i and d.record_offset == len(b"".join(flat[:i]))
    assert D.encode(d.regenerated) == flat[i + 1] and D.encode(d.recovered) == flat[i]
    assert d.epoch_offset == d.offset - len(b"".join(flat[:120]))


def test_timestamp_changed_in_its_last_byte(located):
    flat, t, d = located["flat"], located["timestamp"], located["got"]["timestamp"]
    assert d.kind == "differs" and d.epoch == 2 and d.record == t and d.offset == len(b"".join(flat[:t])) + 8
    assert isinstance(d.regenerated, D.TimestampDeterminant) and isinstance(d.recovered, D.TimestampDeterminant)
    assert d.regenerated.timestamp ^ d.recovered.timestamp == 0x04


def test_log_cut_after_a_whole_record(located):
    flat, d = located["flat"], located["got"]["cut_whole"]
    assert d.kind == "log_is_prefix" and d.record == 300 and d.regenerated is None
    assert D.encode(d.recovered) == flat[300] and d.offset == d.record_offset == len(b"".join(flat[:300]))


def test_log_cut_mid_record(located):
    flat, m, d = located["flat"], located["cut"], located["got"]["cut_mid"]
    assert d.kind == "log_is_prefix" and d.record == m and d.regenerated is None
    assert D.encode(d.recovered) == flat[m] and d.record_offset == len(b"".join(flat[:m])) < d.offset


def test_log_longer_than_the_recovered_one(located):
    d = located["got"]["longer"]
    assert d.kind == "recovered_is_prefix" and d.offset == len(located["whole"]) and d.record == 360
    assert d.recovered is None and d.regenerated == D.OrderDeterminant(3) and d.epoch == 2


def test_from_a_later_epoch(located):
    """Offsets are relative to the range's start."""
    eng, whole = located["eng"], located["whole"]
    log, regen, starts = located["cases"]["swapped"]
    s1 = starts[1]
    (d1,) = locate_divergence(eng, [(log.handle, 1, whole[s1:])])
    assert d1 == expect(regen[s1:], whole[s1:], [-s1, 0, starts[2] - s1])
    assert d1.epoch == 1 and d1.record == located["swapped"] - 120 and d1.offset == located["got"]["swapped"].offset - s1
    assert locate_divergence(eng, []) == []


def test_verify_replay_locate(located):
    """verify_replay(locate=True) carries the same objects; the default call is what it was."""
    eng, items, names = located["eng"], located["items"], located["names"]
    plain = verify_replay(eng, items)
    found = verify_replay(eng, items, locate=True)
    assert [c.matches for c in plain] == [n == "same" for n in names]
    for n, p, c in zip(names, plain, found):
        assert p.divergence is None and (p.matches, p.regenerated, p.recovered) == (c.matches, c.regenerated, c.recovered)
        assert c.divergence == located["want"][n]
