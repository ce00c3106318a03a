"""GPU: the decode at every record split across tile and span ends.  The scenes of
_decode_scenes.py (test_decode_edges_scene.py proves what they cover) go through the three
decode modes -- decode="auto" (the single-launch small path first), "three_pass" (the fast
path) and "robust" -- and every span's records, wide rows and record base, and a batch's first
error, equal the CPU oracle's bit for bit (SimpleDeterminantEncoder.decodeNext, :78-342).
Families A, B, C and E are host input; family D is logs in HBM at segment sizes 16 .. 16384.

Path assertions keep a case from passing only because everything went robust: good batches
without Serializable records on host input or 16 KiB segments stay on the fast path
("three_pass": neither decode_fallback nor decode_span_fallback) and on the single launch
("auto": decode_small without decode_small_fallback); family E's second run, with the
Serializable tables learnt, has no decode_fallback.  At segment sizes of 256 and below short
tiles may go robust by design: the test prints, per segment size, group and mode, whether the
fast path kept the batches."""
import pytest

import _decode_scenes as S
from _decode_util import _raw_decode, as_raw, check_batch_oracle, oracle_batch

pytestmark = pytest.mark.gpu

MODES = ("auto", "three_pass", "robust")

# Scenes that leave the fast path under a rule DESIGN.md states, by name: (family, kind, T,
# record start, note) -> the rule.  Their batches get no path assertion.
EXEMPT = {}

_cache = {}


def _family(name):
    if name not in _cache:
        _cache[name] = {"A": S.family_a, "A_thin": S.family_a_thin, "B": S.family_b, "C": S.family_c,
                        "E": S.family_e}[name]()
    return _cache[name]


def _host_batches(family, T, group):
    """[(scenes, blob, spans, oracle result)] of a family's scenes of one tile size and kind
    group, built once."""
    key = (family, T, group)
    if key not in _cache:
        scenes = [sc for sc in S.by_group(_family(family), {**S.KIND, **S.B_KIND})[group] if sc.T == T]
        out = []
        for b in S.batches([sc for sc in scenes if _exempt_key(sc) not in EXEMPT]) + [
                [sc] for sc in scenes if _exempt_key(sc) in EXEMPT]:
            blob, spans = S.batch(b)
            out.append((b, blob, spans, oracle_batch([sc.span for sc in b])))
        _cache[key] = out
    return _cache[key]


def _exempt_key(sc):
    return (sc.family, sc.kind, sc.T, sc.at, sc.note)


def _launches(ks, name):
    return ks.get(name, {}).get("launches", 0)


class _Engines:
    """The host-input engines of one mode, opened when first used.  Batches with Serializable
    records get an engine of their own: once an engine has met such records it decodes with
    the Serializable tables, and no batch of its takes the single launch any more."""

    def __init__(self, mode):
        self.mode, self.open = mode, {}

    def get(self, ser):
        from clonos_amd import Engine
        if ser not in self.open:
            self.open[ser] = Engine(segment_bytes=16384, pool_segments=64, timing=True, decode=self.mode)
        return self.open[ser]

    def close(self):
        for e in self.open.values():
            e.close()


@pytest.fixture(scope="module", params=MODES)
def engines(request):
    es = _Engines(request.param)
    yield es
    es.close()


def _assert_path(ks, mode, ser, what):
    if mode == "three_pass":
        assert "decode_fallback" not in ks and (ser or "decode_span_fallback" not in ks), (what, sorted(ks))
    if mode == "auto" and not ser:
        assert _launches(ks, "decode_small") == 1 and _launches(ks, "decode_small_fallback") == 0, (what, sorted(ks))
    if mode == "auto" and ser:
        assert "decode_fallback" not in ks, (what, sorted(ks))


GOOD_CASES = ([("A", T, g) for T in S.TILES for g in S.GROUPS] + [("A_thin", T, g) for T in S.TILES for g in S.GROUPS]
              + [("B", S.T_FUSED, g) for g in S.GROUPS] + [("E", S.T_FUSED, "serializable")])


@pytest.mark.parametrize("family,T,group", GOOD_CASES, ids=[f"{f}-{T}-{g}" for f, T, g in GOOD_CASES])
def test_host_scenes(engines, family, T, group):
    """Families A (16-aligned spans, and the thinned variant at blob residues 1..15), B and E:
    every batch equals the oracle, and stays on the path its mode names.  A batch with
    Serializable records runs twice: the first run learns the tables."""
    ser = group == "serializable"
    eng, mode = engines.get(ser), engines.mode
    bs = _host_batches(family, T, group)
    assert bs
    for i, (scenes, blob, spans, exp) in enumerate(bs):
        assert exp["err"] is None
        for rep in range(2 if ser else 1):
            eng.kernel_stats_reset()
            a = _raw_decode(eng, blob, spans)
            check_batch_oracle(a, exp, (family, T, group, mode, i, rep))
        if not any(_exempt_key(sc) in EXEMPT for sc in scenes):
            _assert_path(eng.kernel_stats(), mode, ser, (family, T, group, i))


NEXT_SPAN = S.TAIL  # the good span behind a family-C scene's gap


def _c_scenes(group, pos):
    key = ("C", group, pos)
    if key not in _cache:
        out = []
        for sc in S.by_group(_family("C"))[group]:
            if not sc.note.endswith(" " + pos):
                continue
            blob = sc.span + sc.gap
            blob += bytes(-len(blob) % 16) + NEXT_SPAN
            spans = [(0, len(sc.span)), (len(blob) - len(NEXT_SPAN), len(NEXT_SPAN))]
            out.append((sc, blob, spans, oracle_batch([sc.span, NEXT_SPAN])))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("pos", S.C_POSITIONS)
@pytest.mark.parametrize("group", S.GROUPS)
def test_truncation_alone(engines, group, pos):
    """Family C, every scene in a call of its own: a span that ends inside a record (the
    record's other bytes and more valid records lie right behind it, then the next span), or
    holds an invalid record.  The span keeps the records before the error and only those, the
    next span its own, and status, span, offset and tag of the error are the oracle's."""
    cs = _c_scenes(group, pos)
    assert cs
    eng = engines.get(group == "serializable")
    for sc, blob, spans, exp in cs:
        assert exp["err"] is not None and exp["err"][1] == 0 and exp["err"][2] == sc.at
        check_batch_oracle(_raw_decode(eng, blob, spans), exp, (sc.kind, sc.note, engines.mode))


@pytest.mark.parametrize("group", S.GROUPS)
def test_truncation_batches(engines, group):
    """Family C's mid-tile scenes in batches of many bad spans: each span keeps its records up
    to its own error, and the batch's error is the lowest span's."""
    key = ("Cb", group)
    if key not in _cache:
        scenes = [sc for sc in S.by_group(_family("C"))[group] if sc.note.endswith(" mid")]
        _cache[key] = [(S.batch(b), oracle_batch([sc.span for sc in b])) for b in S.batches(scenes)]
    eng = engines.get(group == "serializable")
    for i, ((blob, spans), exp) in enumerate(_cache[key]):
        assert exp["err"][1] == 0
        check_batch_oracle(_raw_decode(eng, blob, spans), exp, ("C", group, engines.mode, i))


def _d_logs(C, group):
    key = ("D", C, group)
    if key not in _cache:
        logs = [lg for lg in S.d_logs(C) if S.group(S.KIND[lg.kind]) == group]
        _cache[key] = (logs, S.d_batches(logs), [
            [oracle_batch([lg.prefix + lg.body for lg in logs[lo:hi]]), oracle_batch([lg.body for lg in logs[lo:hi]])]
            for lo, hi in S.d_batches(logs)])
    return _cache[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("group", S.GROUPS)
@pytest.mark.parametrize("C", S.SEGMENTS)
def test_logs_in_hbm(C, group, mode):
    """Family D: each log holds an epoch-0 prefix whose length is not a multiple of 16 and the
    scene in epoch 1; decoded from epoch 0 (the whole log) and from epoch 1 (a span that
    starts at an unaligned physical offset)."""
    from clonos_amd import CausalLogID, Engine
    logs, ranges, exps = _d_logs(C, group)
    ser = group == "serializable"
    need = sum((len(lg.prefix) + len(lg.body) + C - 1) // C for lg in logs)
    kept = True
    with Engine(segment_bytes=C, pool_segments=need + 64, timing=True, decode=mode) as e:
        hs = []
        for i, lg in enumerate(logs):
            h = e.open_log(CausalLogID.main(i))
            h.appendDeterminant(lg.prefix, 0)
            h.appendDeterminant(lg.body, 1)
            hs.append(h)
        for (lo, hi), exp in zip(ranges, exps):
            for epoch in (0, 1):
                for rep in range(2 if ser else 1):
                    e.kernel_stats_reset()
                    dec = e.decode_logs(hs[lo:hi], [epoch] * (hi - lo))
                    check_batch_oracle(as_raw(dec), exp[epoch], (C, group, mode, lo, epoch, rep))
                ks = e.kernel_stats()
                if C == 16384:
                    _assert_path(ks, mode, ser, (C, group, lo, epoch))
                kept = kept and "decode_fallback" not in ks and "decode_span_fallback" not in ks
    if mode != "robust":
        print(f"\nfast-path table: segment {C:5d} {group:12s} {mode:10s} "
              f"{'kept' if kept else 'left (robust run for a span or the batch)'}")
