"""Scenes of the decode edge tests (test_gpu_decode_edges.py), free of engine calls: records of
every layout SimpleDeterminantEncoder writes, placed where the decode kernels have special
code -- across tile ends, before short last tiles, cut by span ends, across the segments of
logs, and (Serializable streams) around the phase-3 halo.  test_decode_edges_scene.py checks
the coverage these scenes claim without a GPU.

Conventions: every field value is made of distinct nonzero bytes (a timestamp of
0x0102030405060708), so a dropped, repeated or zeroed byte changes the decoded value.  A scene
is a Scene tuple; a batch is a blob with its spans (offset, length), built by `batch`.

Geometry restated from the C++ (each with its source):

  Tile sizes.  kZTile = 8192 (kernels.h:216) for the single-launch small path and the
  three-pass fast path, kTile = 16384 (kernels.h:24) for the robust path.  kZHalo = 64
  (kernels.h:217), kZJHalo = 1024 (decode_fused.hip:2499).

  Host staging (stage_spans, engine_gather.cpp).  The bytes [lo, hi) of the blob, lo the
  lowest start of a non-empty span and hi the highest end, are copied to the start of one
  device buffer, gaps between spans included.  The buffer is 16-byte aligned, so a span at
  blob offset o is staged at an address whose low four bits are (o - lo) & 15: `delta`.

  Tile plan of a host span (plan_host_span, engine_decode.cpp).  The first tile takes
  T - delta bytes, later tiles T (their delta is 0), the last one what is left.

  Tile window of a log (tile_unit, engine_decode.cpp).  U = min(C, T) when one of C, T
  divides the other, else 0.

  Tile plan of a log span, U != 0 (plan_log_span's device planning, engine_decode.cpp;
  the device expands it).  Tiles are cut at the multiples of U of the physical offset.

  Tile plan of a log span, U == 0 (plan_log_span's host-built tiles, engine_decode.cpp),
  e.g. C = 48.  Tiles are cut per segment, and a segment part longer than T - delta again at
  T - delta.

  Halo branch of a tile (StageGeom, decode_fused.hip:747-763; stage_finish, :795-887).
  after = span offset of the tile's end, halo = min(span length - after, H), H = 64 for the
  count, emit and small kernels and 1024 for phase 3.  With the next tile's descriptor n1 at
  hand, next_ok = halo != 0 and n1 continues the span at `after` and n1.len >= halo.
      near       H <= 64 and next_ok                    one byte per lane
      far16      H > 64 and next_ok and ((hi - n1.delta) & 15) == 0, hi = delta + len
      far_bytes  H > 64 and next_ok, otherwise
      next_long  not next_ok (or no n1), H > 64, halo > 64, the next tile holds the halo
      walk       every other tile with a halo: the walk over the span's tiles
      none       halo == 0: only the zero pad
  Callers (decode_fused.hip): the count pass (:1964), the emit pass (:1635) and the small
  kernel (:2322) pass n1 with H = 64; phase 3 (:2507) passes n1 with H = 1024; the count
  pass's chunk-exit staging (:2142) passes no n1 with H = 64.

  Small path (small_ok, engine_decode.cpp; kSmallBytes, engine_impl.h; kernels.h:471-474).
  A batch of at most 1 MiB, kZSmallSpans = 4096 spans and kZSmallTilesMax = 4096 tiles; a
  plan of at most 64 tiles and 64 spans goes in the kernel argument, a larger one through
  memory.
"""
import struct
from collections import namedtuple

import numpy as np

T_FUSED, T_ROBUST = 8192, 16384
TILES = (T_FUSED, T_ROBUST)
HALO, JHALO = 64, 1024
SPEC_MAX, LM_MAX, CANON_REACH = 256, 126, 2048  # kZSpecMax, kZLmMax, kZCanonLanes * kZRegion
REGION_ROBUST = 256  # kRegion (kernels.h:22)
SMALL_BYTES, SMALL_SPANS, SMALL_TILES, ARG_SPANS, ARG_TILES = 1 << 20, 4096, 4096, 64, 64
SEGMENTS = (16, 32, 48, 64, 256, 16384)


# ---- geometry --------------------------------------------------------------------------------
Tile = namedtuple("Tile", "span_off len delta")


def host_tiles(delta, length, T):
    out, o = [], 0
    while o < length:
        d = (delta + o) & 15
        take = min(length - o, T - d)
        out.append(Tile(o, take, d))
        o += take
    return out


def tile_unit(C, T):
    if C <= T:
        return C if T % C == 0 else 0
    return T if C % T == 0 else 0


def log_tiles(start, length, C, T):
    """Tiles of the span [start, start + length) of a log's physical offsets."""
    out, U = [], tile_unit(C, T)
    if U:
        ph, end = start, start + length
        while ph < end:
            take = min(end - ph, U - ph % U)
            out.append(Tile(ph - start, take, ph & 15))
            ph += take
        return out
    ph, end = start, start + length
    while ph < end:
        so = ph % C
        take, done = min(end - ph, C - so), 0
        while done < take:
            d = (so + done) & 15
            t = min(take - done, T - d)
            out.append(Tile(ph - start + done, t, d))
            done += t
        ph += take
    return out


BRANCHES = ("near", "far16", "far_bytes", "next_long", "walk", "none")
# (name, H, whether the caller passes the next tile's descriptor)
CALLERS = (("count_emit_small", HALO, True), ("chunk_exit", HALO, False), ("phase3", JHALO, True))


def stage_branch(tiles, i, span_len, H, has_n1):
    """The branch stage_finish takes for tile i of a span (tiles: the span's, in order)."""
    td = tiles[i]
    after = td.span_off + td.len
    halo = min(max(span_len - after, 0), H)
    if not halo:
        return "none"
    n1 = tiles[i + 1] if i + 1 < len(tiles) else None
    holds = n1 is not None and n1.span_off == after and n1.len >= halo
    if has_n1 and holds:
        if H <= 64:
            return "near"
        return "far16" if ((td.delta + td.len - n1.delta) & 15) == 0 else "far_bytes"
    if H > 64 and halo > 64 and holds:
        return "next_long"
    return "walk"


# ---- records ----------------------------------------------------------------------------------
MAGIC = b"\xac\xed\x00\x05"


def _pat(n, seed=0):
    """n printable bytes 0x21..0x7e, neighbours distinct."""
    return bytes(0x21 + (i + seed) % 94 for i in range(n))


def order(ch=0x5A):
    return struct.pack(">BB", 0, ch)


def timestamp(v=0x0102030405060708):
    return struct.pack(">BQ", 1, v)


def rng_rec(v=0x11121314):
    return struct.pack(">BI", 2, v)


def buffer_built(v=0x21222324):
    return struct.pack(">BI", 7, v)


def ignore_cp():
    return struct.pack(">BIQ", 6, 0x31323334, 0x4142434445464748)


def timer(ty=3, n=None):
    out = struct.pack(">BIQB", 4, 0x51525354, 0x6162636465666768, ty)
    return out + (struct.pack(">i", n) + _pat(n, 3) if ty == 6 else b"")


def source_cp(n=None, ty=1):
    out = struct.pack(">BIQQBB", 5, 0x71727374, 0x0908070605040302, 0x1918171615141312, ty, 0 if n is None else 1)
    return out + (struct.pack(">i", n) + _pat(n, 5) if n is not None else b"")


def ser_null():
    return b"\x03" + MAGIC + b"\x70"


def ser_string(n):
    return b"\x03" + MAGIC + b"\x74" + struct.pack(">H", n) + _pat(n, 7)


def ser_int_array(k):
    return (b"\x03" + MAGIC + b"\x75\x72\x00\x02[I" + bytes.fromhex("4dba602676eab2a5") + b"\x02\x00\x00\x78\x70"
            + struct.pack(">i", k) + b"".join(struct.pack(">I", 0x01020304 + 0x01010101 * (i % 200)) for i in range(k)))


IA_HDR = len(ser_int_array(0))
LONG_LENGTHS = (125, 126, 127, 255, 256, 257, 2100)
Kind = namedtuple("Kind", "name rec hdr")  # hdr: bytes before the payload (= len(rec) for fixed kinds)


def _kinds():
    ks = [Kind("order", order(), 2), Kind("timestamp", timestamp(), 9), Kind("rng", rng_rec(), 5),
          Kind("buffer_built", buffer_built(), 5), Kind("ignore_cp", ignore_cp(), 13),
          Kind("timer_plain", timer(3), 14), Kind("source_noref", source_cp(None), 23), Kind("ser_null", ser_null(), 6)]
    for n in (0, 1):
        ks += [Kind(f"timer_name_n{n}", timer(6, n), 18), Kind(f"source_ref_n{n}", source_cp(n), 27),
               Kind(f"ser_string_n{n}", ser_string(n), 8), Kind(f"ser_int_array_k{n}", ser_int_array(n), IA_HDR)]
    for L in LONG_LENGTHS:
        ks += [Kind(f"timer_name_L{L}", timer(6, L - 18), 18), Kind(f"source_ref_L{L}", source_cp(L - 27), 27),
               Kind(f"ser_string_L{L}", ser_string(L - 8), 8)]
    for k in (519, 369):  # about 2100 bytes (past the canonical reach) and about 1500 (family E)
        ks.append(Kind(f"ser_int_array_L{IA_HDR + 4 * k}", ser_int_array(k), IA_HDR))
    return ks


KINDS = _kinds()
KIND = {k.name: k for k in KINDS}
for _k in KINDS:
    if "_L" in _k.name:
        assert len(_k.rec) == int(_k.name.rsplit("_L", 1)[1]), _k.name


def is_ser(kind):
    return kind.rec[0] == 3


def group(kind):
    """Kind group of the GPU test's cases."""
    if is_ser(kind):
        return "serializable"
    if len(kind.rec) > 64:
        return "long_timer" if kind.rec[0] == 4 else "long_source"
    return "short"


GROUPS = ("short", "long_timer", "long_source", "serializable")


def split_points(kind):
    """k: tile end k bytes after the record's start.  Every k in 0..L for a record of at most 64
    bytes; for a longer one 0..32 and the payload's first, middle, last and one-past-last byte."""
    L = len(kind.rec)
    if L <= 64:
        return list(range(L + 1))
    return sorted(set(range(33)) | {kind.hdr, kind.hdr + (L - kind.hdr) // 2, L - 1, L})


def starts(kind, T):
    """Record starts of family A: [T - L - 16, T + 16] for a short record; for a long one
    [T - 32 - 16, T + 16] and the named payload positions."""
    L = len(kind.rec)
    if L <= 64:
        return list(range(T - L - 16, T + 17))
    return sorted(set(range(T - 48, T + 17)) | {T - k for k in split_points(kind)})


# ---- filler ---------------------------------------------------------------------------------------
def _var(r, most):
    n = int(r.integers(0, most))
    return struct.pack(">i", n) + _pat(n, int(r.integers(0, 90)))


def _random_record(r, ser):
    t = int(r.integers(0, 9 if ser else 7))
    i = lambda lo, hi: int(r.integers(lo, hi))  # noqa: E731
    if t == 0:
        return order(i(1, 128))
    if t == 1:
        return timestamp(i(1, 1 << 62))
    if t == 2:
        return rng_rec(i(1, 1 << 32))
    if t == 3:
        return buffer_built(i(1, 1 << 31))
    if t == 4:
        ty = i(0, 7)
        return struct.pack(">BIQB", 4, i(0, 1 << 20), i(0, 1 << 45), ty) + (_var(r, 60) if ty == 6 else b"")
    if t == 5:
        has = i(0, 4) != 0
        return struct.pack(">BIQQBB", 5, i(0, 1 << 20), i(0, 1000), i(0, 1 << 45), i(0, 2), int(has)) + (
            _var(r, 80) if has else b"")
    if t == 6:
        return struct.pack(">BIQ", 6, i(0, 1 << 20), i(0, 1000))
    if t == 7:
        return ser_string(i(0, 30))
    return ser_null() if i(0, 2) else ser_int_array(i(0, 8))


N_POOLS = 4
POOL_BYTES = T_ROBUST + 1200


def _pool(seed, ser):
    r = np.random.default_rng(seed)
    parts, ends, at = [], [0], 0
    while at < POOL_BYTES:
        b = _random_record(r, ser)
        parts.append(b)
        at += len(b)
        ends.append(at)
    return b"".join(parts), np.array(ends)


_POOLS = {}


def pool(i, ser=False):
    key = (i % N_POOLS, ser)
    if key not in _POOLS:
        _POOLS[key] = _pool(0xDEC0DE + 17 * key[0] + (1000 if ser else 0), ser)
    return _POOLS[key]


def top_up(g):
    """g bytes of Order and RNG records (g is not 1 or 3)."""
    assert g >= 0 and g not in (1, 3), g
    out = rng_rec() if g % 2 else b""
    return out + order() * ((g - len(out)) // 2)


def filler(n, which=0, ser=False):
    """Exactly n bytes of valid records: a prefix of pool `which`, topped up."""
    if n in (1, 3):
        raise ValueError("no filler of 1 or 3 bytes")
    data, ends = pool(which, ser)
    j = int(np.searchsorted(ends, n, side="right")) - 1
    while n - int(ends[j]) in (1, 3):
        j -= 1
    return data[:int(ends[j])] + top_up(n - int(ends[j]))


TAIL = (timestamp(0x2122232425262728) + order(0x33) + timer(6, 3) + rng_rec(0x41424344) + buffer_built(0x51525354)
        + ignore_cp() + order(0x66) + source_cp(None) + order(0x77))
SER_TAIL = TAIL + ser_string(2) + order(0x12)


# ---- scenes -----------------------------------------------------------------------------------------
# span: the span's bytes.  gap: the unowned bytes behind it in the blob (family C).  kind, T: what
# it aims at.  at: span offset of the record's start.  residue: blob residue the scene is built for
# (its first tile ends at T - residue).  note: what distinguishes it within its family.
Scene = namedtuple("Scene", "family kind T at span gap residue note")


def _scene(family, kind, T, s, which, residue=0, tail=None, ser=None, note=""):
    ser = is_ser(kind) if ser is None else ser
    tail = (SER_TAIL if ser else TAIL) if tail is None else tail
    return Scene(family, kind.name, T, s, filler(s, which, ser and family == "E") + kind.rec + tail, b"", residue, note)


def family_a():
    """Tile-end splits, spans at 16-aligned blob offsets: every kind, each T, every start."""
    out = []
    for q, kind in enumerate(KINDS):
        for T in TILES:
            for i, s in enumerate(starts(kind, T)):
                out.append(_scene("A", kind, T, s, q + i))
    return out


def family_a_thin():
    """Every fourth start of family A (kind q begins at its start q % 4), the residues 1..15
    handed out in turn: a scene built for blob residue r has its record r bytes earlier, since
    its span's first tile ends at T - r."""
    out = []
    for q, kind in enumerate(KINDS):
        for T in TILES:
            for i, s in enumerate(starts(kind, T)[q % 4::4]):
                r = 1 + (i + q) % 15
                if s - r in (1, 3):
                    continue
                out.append(_scene("A", kind, T, s - r, q + i, residue=r, note="thin"))
    return out


B_KINDS = [KIND["timestamp"], KIND["timer_plain"], Kind("timer_name_n3", timer(6, 3), 18),
           Kind("timer_name_n60", timer(6, 60), 18), KIND["source_noref"], Kind("source_ref_n2", source_cp(2), 27),
           Kind("source_ref_n50", source_cp(50), 27), KIND["ser_null"], KIND["ser_string_n1"],
           Kind("ser_string_n70", ser_string(70), 8)]
B_KIND = {k.name: k for k in B_KINDS}
B_R = list(range(1, 33)) + [63, 64, 65]


def family_b():
    """Short last tiles (T = 8192): the span ends r bytes behind the tile end.  "last": the
    record is the span's last, r of its bytes behind the tile end.  "orders": r % 4 of its bytes
    behind the tile end, then Order records up to r."""
    out, T = [], T_FUSED
    for q, kind in enumerate(B_KINDS):
        L = len(kind.rec)
        for r in B_R:
            if r <= L:
                out.append(_scene("B", kind, T, T - (L - r), q + r, tail=b"", note=f"last r={r}"))
            b = r % 4
            if b <= L:
                out.append(_scene("B", kind, T, T - (L - b), q + r, tail=order() * ((r - b) // 2), note=f"orders r={r}"))
    return out


C_POSITIONS = ("mid", "T-1", "T", "T+1", "T+40")


def _c_length(pos):
    return {"mid": 3000, "T-1": T_FUSED - 1, "T": T_FUSED, "T+1": T_FUSED + 1, "T+40": T_FUSED + 40}[pos]


def cuts(kind):
    L = len(kind.rec)
    return [j for j in split_points(kind) if 1 <= j <= L - 1]


def _bad(rec, at, val):
    b = bytearray(rec)
    b[at] = val
    return bytes(b)


def tag_errors():
    """(name, bytes, offset of the error within them is 0): invalid records."""
    neg = struct.pack(">i", -16)
    t6, s1 = timer(6, 4), source_cp(4)
    errs = [("tag8", b"\x08" + rng_rec()[1:]), ("timer_type7", _bad(timer(3), 13, 7)),
            ("timer_typeFF", _bad(timer(3), 13, 0xFF)), ("source_type2", _bad(source_cp(None), 21, 2)),
            ("timer_name_negative", t6[:14] + neg + t6[18:]), ("source_ref_negative", s1[:23] + neg + s1[27:])]
    for m in range(4):
        errs.append((f"ser_magic{m}", _bad(ser_string(3), 1 + m, MAGIC[m] ^ 0x10)))
    return errs


def family_c():
    """Truncation at the span end: the span is filler and the record's first j bytes; the gap
    behind it holds the record's other bytes and further valid records.  And invalid records
    at the same positions (the span goes on behind them; the gap holds valid records)."""
    out = []
    for q, kind in enumerate(KINDS):
        for j in cuts(kind):
            for pos in C_POSITIONS:
                n = _c_length(pos) - j
                sc = _scene("C", kind, T_FUSED, n, q + j, tail=b"", note=f"cut j={j} {pos}")
                out.append(sc._replace(span=sc.span[:n + j], gap=kind.rec[j:] + TAIL))
    for q, (name, rec) in enumerate(tag_errors()):
        for pos in C_POSITIONS:
            # the record's first byte is the span's byte length - 1, ..: its tag is the last
            # byte before position `pos`, so that the bytes it needs lie across it
            n = _c_length(pos) - 1
            out.append(Scene("C", name, T_FUSED, n, filler(n, q) + rec + TAIL, TAIL, 0, f"error {pos}"))
    return out


E_D = list(range(1, 17)) + [1023, 1024, 1025]


def family_e():
    """Serializable streams that start d bytes before the tile end (T = 8192), ending around
    the tile end and around tile end + 1024; the filler holds short Serializable records."""
    out, T = [], T_FUSED

    def add(kind, d, i, note):
        out.append(_scene("E", kind, T, T - d - 1, i, tail=SER_TAIL, ser=True, note=note))

    for i, d in enumerate(E_D):
        for x in sorted({max(7, d + e) for e in (-1, 0, 1)} | {d + JHALO + e for e in (-1, 0, 1)}):
            add(Kind(f"ser_string_S{x}", ser_string(x - 7), 8), d, i + x, f"d={d} stream={x}")
        add(KIND[f"ser_int_array_L{IA_HDR + 4 * 369}"], d, i, f"d={d}")
    for d in range(1, 7):
        add(KIND["ser_null"], d, d, f"d={d}")
    return out


# ---- family D: logs -----------------------------------------------------------------------------------
LOG_MAX = 60000
# prefix: the log's epoch 0 (Order and RNG records, its length's residue mod 16 in 1..15).  body:
# its epoch 1.  starts: physical offsets of the record's starts.
DLog = namedtuple("DLog", "kind prefix body starts")


def d_prefix(i):
    r = 1 + i % 15
    return top_up(r + 16 if r in (1, 3) else r)


def _gap_to(pos, q, m):
    """Smallest g in {0, 2, 4, 5, 6, ..} with (pos + g) % m == q."""
    g = (q - pos) % m
    while g in (1, 3):
        g += m
    return g


def d_small_logs(C):
    """Per kind, logs in which the record recurs, Order and RNG records between, with its
    starts on every residue mod min(C, 64) of the physical offset.  A log ends before LOG_MAX
    bytes, so a long kind takes several."""
    m, out = min(C, 64), []
    for kind in KINDS:
        tail = SER_TAIL if is_ser(kind) else TAIL

        def fresh():
            p = d_prefix(len(out))
            return p, [], len(p), []

        prefix, parts, at, st = fresh()
        for q in list(range(m)) + [0]:
            g = _gap_to(at, q, m)
            if st and at + g + len(kind.rec) + len(tail) > LOG_MAX:
                out.append(DLog(kind.name, prefix, b"".join(parts) + tail, st))
                prefix, parts, at, st = fresh()
                g = _gap_to(at, q, m)
            parts += [top_up(g), kind.rec]
            st.append(at + g)
            at += g + len(kind.rec)
        out.append(DLog(kind.name, prefix, b"".join(parts) + tail, st))
    return out


def d_big_logs():
    """16 KiB segments: the family-A placements of both tile sizes as logs -- record starts
    around the physical offsets 8192 (a tile end of the fused paths inside a segment) and
    16384 (a segment end, and the robust path's tile end)."""
    out = []
    for q, kind in enumerate(KINDS):
        tail = SER_TAIL if is_ser(kind) else TAIL
        for T in TILES:
            for i, s in enumerate(starts(kind, T)):
                p = d_prefix(len(out))
                out.append(DLog(kind.name, p, filler(s - len(p), q + i) + kind.rec + tail, [s]))
    return out


def d_logs(C):
    return d_big_logs() if C == 16384 else d_small_logs(C)


def d_batches(logs, limit=SMALL_BYTES - 65536):
    """Index ranges of the logs of one decode call, as `batches` cuts them."""
    out, lo, size = [], 0, 0
    for i, l in enumerate(logs):
        n = len(l.prefix) + len(l.body)
        if i > lo and (size + n > limit or (not out and i - lo == FIRST_BATCH)):
            out.append((lo, i))
            lo, size = i, 0
        size += n
    out.append((lo, len(logs)))
    return out


# ---- batches ------------------------------------------------------------------------------------------
def batch(scenes):
    """(blob, spans, delta per span): spans in order, each at the next blob offset whose low
    four bits are its scene's residue (the first span's offset is the staging base, so that is
    its delta), the scene's gap behind it."""
    parts, spans, at = [], [], 0
    for i, sc in enumerate(scenes):
        o = (at + 15) // 16 * 16 + (sc.residue if i else 0)
        parts.append(bytes(o - at) + sc.span + sc.gap)
        spans.append((o, len(sc.span)))
        at = o + len(sc.span) + len(sc.gap)
    return b"".join(parts), spans


def batch_deltas(scenes):
    return [sc.residue if i else 0 for i, sc in enumerate(scenes)]


def n_tiles(scenes, T=T_FUSED):
    return sum(len(host_tiles(d, len(sc.span), T)) for sc, d in zip(scenes, batch_deltas(scenes)))


FIRST_BATCH = 20  # spans of a group's first batch: at most 64 tiles, the kernel-argument plan form


ANCHOR = Scene("A", "anchor", T_FUSED, 0, TAIL, b"", 0, "anchor")


def batches(scenes, limit=SMALL_BYTES - 65536):
    """Scenes in order in batches of at most `limit` blob bytes; the first holds FIRST_BATCH.
    A batch whose first scene is built for a residue starts with ANCHOR, a short span at blob
    offset 0: the first span's delta is always 0."""
    out, cur, size = [], [], 0
    for sc in scenes:
        n = len(sc.span) + len(sc.gap) + 32
        if cur and (size + n > limit or (not out and len(cur) == FIRST_BATCH)):
            out.append(cur)
            cur, size = [], 0
        if not cur and sc.residue:
            cur.append(ANCHOR)
        cur.append(sc)
        size += n
    if cur:
        out.append(cur)
    return out


def by_group(scenes, kinds=None):
    kinds = kinds or KIND
    out = {g: [] for g in GROUPS}
    for sc in scenes:
        k = kinds.get(sc.kind)
        if k is None:  # family E's strings, family C's invalid records, the anchor
            g = "serializable" if sc.kind.startswith("ser_") else "short"
        else:
            g = group(k)
        out[g].append(sc)
    return out
