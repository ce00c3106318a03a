"""Scenes of the batched encode's edge tests (test_gpu_encode_edges.py), free of engine calls:
records built by hand in the decode's SoA layout (no decoder involved), the places they are put
at, and the lowest bad record of every validation scene.  test_encode_edges_scene.py checks the
coverage these scenes claim with the oracle alone.

A batch is the tuple Engine.encode_batch and _oracle.encode_soa take:
(tag, v0, w_idx, w_rc, w_v1, w_var_off, w_var_len, w_sub, var).

Conventions: payload bytes are drawn from 1..254 and output buffers hold FILL (0xFF), so a
misplaced payload byte cannot look like fill or zero.  The constants are encode.hip's: a block
of BLOCK records, PER records per thread, WAVE records per wavefront, an LDS stage of STAGE
bytes (a block whose bytes are at most STAGE is staged, a larger one stores directly).
"""
import numpy as np

FILL = 0xFF
BLOCK, PER, WAVE, STAGE = 1024, 4, 256, 28 * 1024
SCAN = 1024  # blocks per round of k_enc_scan / k_enc_scan64

NARROW = ("order", "timestamp", "rng", "buffer_built")
WIDE = ("ignore", "timer6_empty", "timer6_name", "timer_other", "source_plain", "source_ref_empty", "source_ref",
        "serial_empty", "serial")
KINDS = NARROW + WIDE  # the ten determinant kinds, with the payload variants of three of them
TAG = {"order": 0, "timestamp": 1, "rng": 2, "buffer_built": 7, "ignore": 6, "timer6_empty": 4, "timer6_name": 4,
       "timer_other": 4, "source_plain": 5, "source_ref_empty": 5, "source_ref": 5, "serial_empty": 3, "serial": 3}

I8 = (-(1 << 7), (1 << 7) - 1, -1, 0)
I32 = (-(1 << 31), (1 << 31) - 1, -1, 0)
I64 = (-(1 << 63), (1 << 63) - 1, -1, 0)
# v0 with bits above the field's width (the encoder's casts drop them): the low byte / word is
# 0x80.. / 0x7F.., so a sign extension or a saturation would show
ABOVE8 = (0x0102030405060780, -0x0102030405060781, 0x100, 0x17F)
ABOVE32 = (0x0102030480000000, -0x0102030480000001, 1 << 32, 0x17FFFFFFF)
TIMER_SUBS = tuple(range(7))          # TimerService callback ordinals the decode accepts
SOURCE_SUBS = (0, 1, 0x80, 0x81)      # checkpoint type 0 / 1, with and without a storage reference


def payload(rng, n):
    return rng.integers(1, 255, n, dtype=np.uint8).tobytes()


def has_payload(tag, sub):
    """The format carries a payload for this wide row."""
    return tag == 3 or (tag == 4 and sub == 6) or (tag == 5 and bool(sub & 0x80))


def rec_len(tag, sub=0, var_len=0):
    """Encoded bytes of one record (SimpleDeterminantEncoder.java:124-323)."""
    fixed = {0: 2, 1: 9, 2: 5, 7: 5, 6: 13, 3: 1, 4: 18 if sub == 6 else 14, 5: 27 if sub & 0x80 else 23}[tag]
    return fixed + (var_len if has_payload(tag, sub) else 0)


class Batch:
    """Records appended one by one; every field not given is drawn from its whole width."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.tag, self.v0, self.side, self.var, self.kinds = [], [], [], bytearray(), []

    def add(self, kind, v0=None, rc=None, v1=None, sub=None, data=None, n_data=None):
        r, t, i = self.rng, TAG[kind], len(self.tag)
        if v0 is None:
            v0 = int(r.integers(-(1 << 63), (1 << 63) - 1)) if t in (1, 4, 5, 6) else \
                int(r.integers(-128, 128)) if t == 0 else int(r.integers(-(1 << 31), 1 << 31))
        self.tag.append(t), self.v0.append(v0), self.kinds.append(kind)
        if kind in NARROW:
            return self
        rc = int(r.integers(-(1 << 31), 1 << 31)) if rc is None else rc
        v1 = (int(r.integers(-(1 << 63), (1 << 63) - 1)) if t == 5 else 0) if v1 is None else v1
        if sub is None:
            sub = {"timer6_empty": 6, "timer6_name": 6, "timer_other": int(r.integers(0, 6)),
                   "source_plain": int(r.integers(0, 2)), "source_ref_empty": 0x80 | int(r.integers(0, 2)),
                   "source_ref": 0x80 | int(r.integers(0, 2))}.get(kind, 0)
        if data is None:
            if n_data is None:
                n_data = int(r.integers(1, 41)) if kind in ("timer6_name", "source_ref", "serial") else 0
            data = payload(r, n_data)
        assert has_payload(t, sub) or not data
        self.side.append((i, rc, v1, len(self.var), len(data), sub))
        self.var += data
        return self

    def soa(self):
        cols = list(zip(*self.side)) if self.side else [[]] * 6
        wrap = lambda xs, bits, t: np.array([x & ((1 << bits) - 1) for x in xs], np.uint64).astype(t)  # noqa: E731
        return (np.array(self.tag, np.uint8), wrap(self.v0, 64, np.int64), np.array(cols[0], np.uint32),
                wrap(cols[1], 32, np.int32), wrap(cols[2], 64, np.int64), np.array(cols[3], np.uint32),
                np.array(cols[4], np.uint32), np.array(cols[5], np.uint8), bytes(self.var))


def of_kinds(kinds, seed):
    b = Batch(seed)
    for k in kinds:
        b.add(k)
    return b.soa()


def lens_of(soa):
    """Encoded length of every record, from the rows alone."""
    tag, _, w_idx, _, _, _, w_len, w_sub, _ = soa
    out = np.array([rec_len(int(t)) if int(t) in (0, 1, 2, 7) else 0 for t in tag], np.int64)
    for k, i in enumerate(w_idx):
        out[int(i)] = rec_len(int(tag[int(i)]), int(w_sub[k]), int(w_len[k]))
    return out


def cut(soa, a, b):
    """Records [a, b) as a batch of their own (side rows renumbered; var kept whole)."""
    tag, v0, w_idx, w_rc, w_v1, w_off, w_len, w_sub, var = soa
    m = (w_idx >= a) & (w_idx < b)
    return (tag[a:b], v0[a:b], (w_idx[m] - a).astype(np.uint32), w_rc[m], w_v1[m], w_off[m], w_len[m], w_sub[m], var)


def wide_blocks(soa):
    """The blocks that hold a wide record."""
    return sorted({int(i) // BLOCK for i in soa[2]})


# ---- lengths --------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
MIXES = ("narrow", "wide", "cycle")


def mix_kinds(mix, n, which=0):
    """narrow: the four narrow kinds at random; wide: n records of one wide kind; cycle: every
    kind in turn (a period of 13, coprime to the 4 records of a thread)."""
    if mix == "narrow":
        r = np.random.default_rng(1000 + n)
        return [NARROW[int(x)] for x in r.integers(0, 4, n)]
    if mix == "wide":
        return [WIDE[which % len(WIDE)]] * n
    return [KINDS[(i + which) % len(KINDS)] for i in range(n)]


def length_scenes():
    """(mix, n, batch)."""
    return [(mix, n, of_kinds(mix_kinds(mix, n, j), 2000 + 16 * MIXES.index(mix) + j))
            for mix in MIXES for j, n in enumerate(LENGTHS)]


# ---- every kind at every slot of a thread and at the seams -------------------------------------------
SLOT_AT = (8, 13, 18, 23)  # record i mod 4 = 0, 1, 2, 3, each between records of another kind
SEAMS = {"wave": (255, 256), "block": (1023, 1024), "block2": (2047, 2048)}
PLACE_N = 2 * BLOCK + 3


def place_positions(side):
    """Where the kind under test stands: side 0 holds the slots and the last record before each
    seam, side 1 the first record after it, so both neighbours are of the other kind."""
    return sorted((SLOT_AT if side == 0 else ()) + tuple(s[side] for s in SEAMS.values()))


def place_kinds(kind, side):
    """The kind under test among records of another kind: a wide one around a narrow kind and a
    narrow one around a wide kind, so the wide prefix changes at the very record."""
    other = "ignore" if kind in NARROW else "order"
    at = set(place_positions(side))
    return [kind if i in at else other for i in range(PLACE_N)]


def place_scenes():
    """(kind, side, batch)."""
    return [(k, s, of_kinds(place_kinds(k, s), 3000 + 2 * j + s)) for j, k in enumerate(KINDS) for s in (0, 1)]


def place_coverage(kinds):
    """(kind, slot) and (kind, seam, side) of every record whose two neighbours are of another kind."""
    slots, seams = set(), set()
    for i, k in enumerate(kinds):
        if (i and kinds[i - 1] == k) or (i + 1 < len(kinds) and kinds[i + 1] == k):
            continue
        slots.add((k, i % PER))
        for name, pair in SEAMS.items():
            if i in pair:
                seams.add((k, name, pair.index(i)))
    return slots, seams


# ---- the wide-row prefix ------------------------------------------------------------------------------
def prefix_scenes():
    """(name, batch): a block of 1024 wide records (then a second block); wide records only at the
    last record of a block and the first of a later one, blocks without any between; one wide
    record as the very last."""
    full = [WIDE[i % len(WIDE)] for i in range(BLOCK)] + [KINDS[i % len(KINDS)] for i in range(7)]
    n = 5 * BLOCK + 3
    at = {BLOCK - 1: "timer6_name", 3 * BLOCK: "source_ref", 4 * BLOCK - 1: "ignore", 4 * BLOCK: "serial"}
    gaps = [at.get(i, NARROW[i % 3]) for i in range(n)]
    last = [NARROW[i % 4] for i in range(1500)] + ["source_ref"]
    return [("full_block", of_kinds(full, 4000)), ("empty_blocks", of_kinds(gaps, 4001)),
            ("last", of_kinds(last, 4002))]


# ---- field extremes ---------------------------------------------------------------------------------
def extremes():
    """Every field at the min, max, -1 and 0 of its width, v0 with bits above its width, both
    flag states and every checkpoint type and callback ordinal."""
    b = Batch(5000)
    for v in I8 + ABOVE8:
        b.add("order", v0=v)
    for v in I64:
        b.add("timestamp", v0=v)
    for v in I32 + ABOVE32:
        b.add("rng", v0=v)
        b.add("buffer_built", v0=v)
    for v in I64:
        for rc in I32:
            b.add("ignore", v0=v, rc=rc)
    for sub in TIMER_SUBS:
        for rc in I32:
            for v in I64:
                b.add("timer6_name" if sub == 6 else "timer_other", v0=v, rc=rc, sub=sub)
        if sub == 6:
            b.add("timer6_empty", sub=6)
    for sub in SOURCE_SUBS:
        for v1 in I64:
            for k, v in enumerate(I64):
                b.add("source_ref" if sub & 0x80 else "source_plain", v0=v, rc=I32[k], v1=v1, sub=sub)
        if sub & 0x80:
            b.add("source_ref_empty", sub=sub)
    for v in I64:  # (a Serializable's v0 is not encoded)
        b.add("serial", v0=v)
    b.add("serial_empty")
    return b.soa()


# ---- the stage limit -----------------------------------------------------------------------------------
STAGE_L = (STAGE - 2047 - 1, STAGE - 2047, STAGE - 2047 + 1)  # block totals 28 671, 28 672, 28 673
assert STAGE_L == (26624, 26625, 26626)


def long_block(b, L, at):
    """One block: 1023 Orders and a Serializable of L bytes as its record `at`."""
    for i in range(BLOCK):
        if i == at:
            b.add("serial", n_data=L)
        else:
            b.add("order")


def stage_scenes():
    """(name, batch, expected block totals)."""
    out = []
    for L in STAGE_L:
        for name, at in (("mid", 500), ("first", 0), ("last", BLOCK - 1)):
            b = Batch(6000 + L + at)
            long_block(b, L, at)
            out.append((f"{name}_{2047 + L}", b.soa(), [2047 + L]))
    b = Batch(6100)  # staged at the limit | direct | a block of one record
    long_block(b, STAGE_L[1], BLOCK - 1)
    long_block(b, STAGE_L[2], BLOCK - 1)
    b.add("timer6_name", n_data=5)
    out.append(("staged_direct_one", b.soa(), [STAGE, STAGE + 1, 23]))
    for extra in (0, 1):  # the limit reached by many medium payloads: 1024 names of 9 / 11 bytes
        b = Batch(6200 + extra)
        for i in range(BLOCK):
            b.add("timer6_name", n_data=(9 if i % 2 == 0 else 11) + (extra if i == BLOCK - 1 else 0))
        for k in ("order", "serial", "rng"):
            b.add(k, n_data=3 if k == "serial" else None)
        out.append((f"names_{STAGE + extra}", b.soa(), [STAGE + extra, 2 + 4 + 5]))
    return out


# ---- the second round of the scans -------------------------------------------------------------------
SCAN_BLOCKS = SCAN + 3                   # 1027 blocks, the last of one record
SCAN_N = (SCAN + 2) * BLOCK + 1
SCAN_WIDE_BLOCKS = (0, SCAN - 1, SCAN, SCAN + 1, SCAN + 2)


def scan_round():
    """Narrow records, and fixed-width wide records (IgnoreCheckpoint, TimerTrigger without a name,
    SourceCheckpoint without a reference) in the first block, the last of the first round, the
    first two of the second and the last: every wide record after block 1023 finds its row, and
    every byte after it its place, only through the carry of both scans."""
    r = np.random.default_rng(7000)
    tag = np.array([0, 1, 2, 7], np.uint8)[r.integers(0, 4, SCAN_N)]
    v0 = r.integers(-(1 << 63), (1 << 63) - 1, SCAN_N, dtype=np.int64)
    at = [b * BLOCK + o for b in SCAN_WIDE_BLOCKS for o in (0, 5, BLOCK - 1) if b * BLOCK + o < SCAN_N]
    kinds = [(6, 0), (4, 2), (5, 1), (4, 5), (5, 0)]
    w_tag = np.array([kinds[k % 5][0] for k in range(len(at))], np.uint8)
    tag[at] = w_tag
    w_sub = np.array([kinds[k % 5][1] for k in range(len(at))], np.uint8)
    w_rc = r.integers(-(1 << 31), 1 << 31, len(at)).astype(np.int32)
    w_v1 = r.integers(-(1 << 63), (1 << 63) - 1, len(at), dtype=np.int64)
    zero = np.zeros(len(at), np.uint32)
    return (tag, v0, np.array(at, np.uint32), w_rc, w_v1, zero, zero.copy(), w_sub, b"")


# ---- validation ------------------------------------------------------------------------------------
def first_bad(soa, var_len=None):
    """What clg_encode_batch reports in *bad_index (None: the batch is valid): the lowest record
    with a tag above 7, a wide record without a side row or whose row names another record or
    whose payload range passes var; n when every record is valid and rows are left over."""
    tag, _, w_idx, _, _, w_off, w_len, w_sub, var = soa
    var_len = len(var) if var_len is None else var_len
    w = 0
    for i in range(len(tag)):
        t = int(tag[i])
        if t > 7:
            return i
        if 3 <= t <= 6:
            if w >= len(w_idx) or int(w_idx[w]) != i:
                return i
            if has_payload(t, int(w_sub[w])) and int(w_off[w]) + int(w_len[w]) > var_len:
                return i
            w += 1
    return len(tag) if w != len(w_idx) else None


def valid_batch():
    return of_kinds(mix_kinds("cycle", 2 * BLOCK + 2), 8000)


def _copy(soa):
    return tuple(a.copy() if isinstance(a, np.ndarray) else a for a in soa)


def _rows(soa, keep):
    return soa[:2] + tuple(a[keep] for a in soa[2:8]) + soa[8:]


def validation_scenes():
    """(name, batch, lowest bad record)."""
    base = valid_batch()
    n, out = len(base[0]), []

    def put(name, s):
        out.append((name, s, first_bad(s)))

    for bad in (8, 255):
        for pos in (0, BLOCK - 1, BLOCK, n - 1):
            s = _copy(base)
            s[0][pos] = bad
            put(f"tag{bad}_at_{pos}", s)
    s = _copy(base)
    s[0][1500], s[0][300] = 8, 9
    put("two_blocks", s)
    s = _copy(base)
    s[0][40], s[0][42] = 8, 8
    put("one_thread", s)
    in_block = np.flatnonzero((base[2] >= BLOCK) & (base[2] < 2 * BLOCK))
    for name, k in (("first", int(in_block[0])), ("last", int(in_block[-1]))):
        s = _copy(base)
        s[2][k] += 1
        put(f"row_names_another_{name}", s)
    nw = len(base[2])
    put("one_row_too_few", _rows(base, np.arange(nw - 1)))
    put("one_row_too_many", _rows(base, np.concatenate([np.arange(nw), [nw - 1]])))
    s = _copy(base)
    p = next(int(i) for i in base[2] if int(i) % PER < PER - 1 and int(i) > BLOCK)
    s[0][p + 1] = 8
    put("after_wide_in_thread", s)
    return out


# ---- payload ranges ----------------------------------------------------------------------------------
def range_batch():
    """Payload rows of each format; the last payload (a Serializable's) ends on var's last byte,
    and an empty Serializable follows at offset var_len."""
    b = Batch(9000)
    for k in ("order", "timer6_name", "ignore", "source_ref", "timer_other", "rng", "source_plain", "serial",
              "serial_empty", "timestamp"):
        b.add(k)
    return b.soa()


def range_scenes():
    """(name, batch, lowest bad record or None, the batch whose bytes a valid one encodes to)."""
    base = range_batch()
    tag, w_idx, w_off, w_len, var = base[0], base[2], base[5], base[6], base[8]
    k_last = next(k for k in range(len(w_idx)) if int(w_off[k]) + int(w_len[k]) == len(var) and int(w_len[k]))
    k_empty = next(k for k in range(len(w_idx)) if int(tag[int(w_idx[k])]) == 3 and not int(w_len[k]))
    assert int(w_off[k_empty]) == len(var)
    out = [("exact", base, None, base)]
    for over in (1, 8):
        s = _copy(base)
        s[6][k_last] += over
        out.append((f"over_by_{over}", s, int(w_idx[k_last]), None))
    s = _copy(base)
    s[5][k_empty] = len(var) + 1
    out.append(("empty_past_the_end", s, int(w_idx[k_empty]), None))
    s = _copy(base)
    for k, i in enumerate(w_idx):  # rows whose format carries no payload: never read
        if not has_payload(int(tag[int(i)]), int(base[7][k])):
            s[5][k], s[6][k] = 0xFFFFFFF0, 0xFFFFFFFF
    out.append(("wild_without_payload", s, None, base))
    return out
