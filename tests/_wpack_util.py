"""Shared by the packed-wide-rows tests: an independent numpy packer of the format in
clonos_amd/csrc/pack_wide.h (its own copy of the stream table, the partition by boolean masks, a
block through _pack_util.pack_block, which shares no code with the library), hand-made wide rows
and helpers to compare a PackedWide with the numpy packer or with another PackedWide."""
import numpy as np

from _pack_util import BLOCK, DESC, pack_block, values_of_width

KINDS, FIELDS, STREAMS = 4, 6, 26
# the six fields of a kind's rows: the clg_columns array, what it is extended from, DELTA for kind 0,
# DELTA for kinds 1 - 3
FIELD = (("w_rc", np.int32, False, False), ("w_v1", np.int64, True, True), ("w_var_off", np.uint32, True, True),
         ("w_var_len", np.uint32, False, False), ("w_sub", np.uint8, False, False), ("w_v0", np.int64, False, True))
WIDE = ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")
WIDE_DT = (np.uint32, np.int32, np.int64, np.uint32, np.uint32, np.uint8, np.int64)
PLAIN_ROW_BYTES = 33  # the seven arrays, a row


def stream_values(cols):
    """The 26 streams of cols' wide rows: (values in their own dtype, delta) each."""
    tag = np.asarray(cols.tag, np.uint8)
    idx = np.asarray(cols.w_idx, np.uint32)
    kind = (tag[idx].astype(np.int64) - 3).astype(np.uint8) if idx.size else np.zeros(0, np.uint8)
    assert (kind < KINDS).all()
    out = [(kind, False), (idx, True)]
    for t in range(KINDS):
        sel = kind == t
        for name, dt, d0, d in FIELD:
            out.append((np.ascontiguousarray(getattr(cols, name), dt)[sel], d if t else d0))
    return out


def pack_numpy(cols):
    """desc rows, the payload bytes, n_val and blk_base of the wide rows of `cols`."""
    rows, chunks, n_val, blk_base, pos = [], [], [], [0], 0
    for x, delta in stream_values(cols):
        n_val.append(int(x.size))
        for i0 in range(0, x.size, BLOCK):
            blk = x[i0:i0 + BLOCK]
            ref, first, width, payload = pack_block(blk, delta)
            rows.append((ref, first, pos, width, blk.size))
            chunks.append(payload)
            pos += len(payload)
        blk_base.append(len(rows))
    return np.array(rows, DESC) if rows else np.zeros(0, DESC), b"".join(chunks), n_val, blk_base


def assert_wide_equals_numpy(packed, cols):
    desc, bits, n_val, blk_base = pack_numpy(cols)
    assert packed.n_val == n_val and packed.blk_base == blk_base
    got = np.asarray(packed.desc)
    for f in DESC.names:
        assert (got[f] == desc[f]).all(), f
    assert np.asarray(packed.bits).tobytes() == bits


def assert_same_wide(a, b):
    """Two PackedWide hold the same descriptors and bits, byte for byte."""
    assert a.n_val == b.n_val and a.blk_base == b.blk_base
    assert np.asarray(a.desc).tobytes() == np.asarray(b.desc).tobytes()
    assert np.asarray(a.bits).tobytes() == np.asarray(b.bits).tobytes()


def assert_round_trip(packed, cols):
    back = packed.unpack()
    for name, dt in zip(WIDE, WIDE_DT):
        a, b = back[name], np.asarray(getattr(cols, name), dt)
        assert a.dtype == dt and a.shape == b.shape and (a == b).all(), name


def plain_bytes(cols):
    return PLAIN_ROW_BYTES * len(cols.w_idx)


class Wide:
    """Wide rows by hand, shaped like DecodedColumns for the wide pack: `kinds` names each row's
    kind; every wide record sits behind `gap` narrow records, so w_idx climbs by gap + 1."""

    def __init__(self, kinds, gap=1, **fields):
        kinds = np.asarray(kinds, np.uint8)
        n = kinds.size
        self.tag = np.zeros(n * (gap + 1), np.uint8)
        self.w_idx = (np.arange(n, dtype=np.uint32) * (gap + 1) + gap).astype(np.uint32)
        self.tag[self.w_idx] = kinds + 3
        for name, dt in zip(WIDE[1:], WIDE_DT[1:]):
            a = np.asarray(fields.get(name, np.zeros(n, dt)), dt)
            assert a.shape == (n,), name
            setattr(self, name, a)
        self.order, self.timestamp = np.zeros(0, np.int8), np.zeros(0, np.int64)
        self.rng, self.buffer_built = np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.span_base = np.zeros((1, 5), np.uint64)
        self.spans_bytes = self.var = self.var_pos = self.error = None


def seeded_wide(kinds, seed, gap=1):
    """Believable rows: counters, clocks that advance, offsets that climb, small lengths."""
    rng = np.random.default_rng(seed)
    kinds = np.asarray(kinds, np.uint8)
    n = kinds.size
    clock = 1_700_000_000_000 + np.cumsum(rng.integers(0, 50, n))
    v0 = np.where(kinds == 0, rng.integers(0, 300, n), np.where(kinds == 1, clock - 7, 40 + np.arange(n)))
    return Wide(kinds, gap, w_rc=rng.integers(0, 1 << 31, n), w_v1=np.where(kinds == 0, 0, clock),
                w_var_off=np.cumsum(rng.integers(9, 60, n)), w_var_len=rng.integers(0, 300, n),
                w_sub=rng.integers(0, 3, n), w_v0=v0)


def offsets_of_width(rng, width, n):
    """n >= 3 u32 values whose DELTA residuals span exactly `width` <= 32 bits: a walk whose steps
    lie in [-2^(width-1), 2^(width-1) - 1], both ends present, each step drawn from the part of that
    range that keeps the value a u32 (it always holds 0)."""
    if width == 0:
        return (1 << 31) + 7 * np.arange(n, dtype=np.int64)  # a constant step
    lo, hi = -(1 << (width - 1)), (1 << (width - 1)) - 1
    x = [1 << 31, (1 << 31) + lo, (1 << 31) + lo + hi]
    while len(x) < n:
        x.append(x[-1] + int(rng.integers(max(lo, -x[-1]), min(hi, 2 ** 32 - 1 - x[-1]), endpoint=True)))
    return np.array(x[:n], np.int64)


def width_scene(width, n=1024, seed=0):
    """n rows of every kind in turn (4 n rows: kind k's rows are one block when n is 1024) whose
    streams have exactly these widths: `width` on the i64 fields, min(width, 32) on RC, VAR_OFF and
    VAR_LEN, min(width, 8) on SUB."""
    rng = np.random.default_rng(0x51DE + 977 * width + seed)
    w32, w8 = min(width, 32), min(width, 8)
    kinds = np.repeat(np.arange(KINDS, dtype=np.uint8), n)
    f = {k: [] for k in WIDE[1:]}
    for t in range(KINDS):
        f["w_rc"].append(values_of_width(rng, np.int32, w32, n))
        f["w_v1"].append(values_of_width(rng, np.int64, width, n, delta=True))
        f["w_var_off"].append(offsets_of_width(rng, w32, n))
        f["w_var_len"].append(values_of_width(rng, np.int64, w32, n, vmin=0, vmax=(1 << 32) - 1))
        f["w_sub"].append(values_of_width(rng, np.uint8, w8, n))
        f["w_v0"].append(values_of_width(rng, np.int64, width, n, delta=t > 0))
    return Wide(kinds, **{k: np.concatenate(v) for k, v in f.items()})


def widths_of(packed, kind):
    """The first block's width of each field's stream of `kind`, in FIELD's order."""
    return [int(packed.desc["width"][packed.blk_base[2 + FIELDS * kind + f]]) for f in range(FIELDS)]
