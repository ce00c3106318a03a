"""Shared by the packed-columns tests: an independent numpy packer of the format in
clonos_amd/csrc/pack.h (it shares no code with the library: residuals and the reference by array
arithmetic, the payload through a bit matrix and np.packbits), and helpers to compare a
PackedColumns with it."""
import numpy as np

BLOCK = 1024
STREAMS = (("tag", np.uint8, False), ("order", np.int8, False), ("timestamp", np.int64, True),
           ("rng", np.int32, False), ("buffer_built", np.int32, False))
DESC = np.dtype([("ref", np.int64), ("first", np.int64), ("pos", np.uint64), ("width", np.uint32), ("count", np.uint32)])


def pack_block(x, delta):
    """(ref, first, width, payload bytes) of one block of values x (its own dtype)."""
    v = np.asarray(x).astype(np.int64).view(np.uint64)  # sign-extended (u8 zero-extended), as raw 64 bits
    first = 0
    if delta:
        first = int(np.asarray(x).astype(np.int64)[0])
        r = v[1:] - v[:-1]  # modulo 2^64
    else:
        r = v
    if r.size == 0:
        return 0, first, 0, b""
    rs = r.view(np.int64)
    ref, top = int(rs.min()), int(rs.max())
    rng = (top - ref) & 0xFFFFFFFFFFFFFFFF
    width = rng.bit_length()
    if width == 0:
        return ref, first, 0, b""
    p = r - np.uint64(ref & 0xFFFFFFFFFFFFFFFF)
    assert int(p.max()) < (1 << width)
    bit = ((p[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    pad = (-bit.size) % 128
    bit = np.concatenate([bit, np.zeros(pad, np.uint8)])
    return ref, first, width, np.packbits(bit, bitorder="little").tobytes()


def pack_numpy(cols):
    """desc rows, the payload bytes, n_val and blk_base of the five narrow columns of `cols`
    (anything with tag / order / timestamp / rng / buffer_built arrays)."""
    rows, chunks, n_val, blk_base, pos = [], [], [], [0], 0
    for name, dt, delta in STREAMS:
        x = np.ascontiguousarray(getattr(cols, name), dt)
        n_val.append(x.size)
        for i0 in range(0, x.size, BLOCK):
            blk = x[i0:i0 + BLOCK]
            ref, first, width, payload = pack_block(blk, delta)
            rows.append((ref, first, pos, width, blk.size))
            chunks.append(payload)
            pos += len(payload)
        blk_base.append(len(rows))
    return np.array(rows, DESC) if rows else np.zeros(0, DESC), b"".join(chunks), n_val, blk_base


def assert_packed_equals_numpy(packed, cols):
    desc, bits, n_val, blk_base = pack_numpy(cols)
    assert packed.n_val == n_val and packed.blk_base == blk_base
    got = np.asarray(packed.desc)
    for f in DESC.names:
        assert (got[f] == desc[f]).all(), f
    assert np.asarray(packed.bits).tobytes() == bits


def assert_same_packed(a, b):
    """Two PackedColumns hold the same descriptors and bits, byte for byte."""
    assert a.n_val == b.n_val and a.blk_base == b.blk_base
    assert np.asarray(a.desc).tobytes() == np.asarray(b.desc).tobytes()
    assert np.asarray(a.bits).tobytes() == np.asarray(b.bits).tobytes()


class Narrow:
    """Five narrow columns by hand (the wide rows empty), shaped like DecodedColumns for the pack."""

    def __init__(self, tag=(), order=(), timestamp=(), rng=(), buffer_built=()):
        self.tag, self.order = np.asarray(tag, np.uint8), np.asarray(order, np.int8)
        self.timestamp, self.rng = np.asarray(timestamp, np.int64), np.asarray(rng, np.int32)
        self.buffer_built = np.asarray(buffer_built, np.int32)
        self.w_idx, self.w_rc, self.w_v1 = np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int64)
        self.w_var_off, self.w_var_len = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        self.w_sub, self.w_v0 = np.zeros(0, np.uint8), np.zeros(0, np.int64)
        self.span_base = np.zeros((1, 5), np.uint64)
        self.spans_bytes = self.var = self.var_pos = self.error = None


def values_of_width(rng, dtype, width, n, delta=False, vmin=None, vmax=None):
    """n values of `dtype` whose block residuals (the values, or with delta their differences)
    span exactly `width` bits: the lowest and the highest residual are both present.  Without delta
    the values stay in [vmin, vmax] (the type's limits by default); with delta n must be at
    least 3 for a width above 0 (two residuals)."""
    M = 0xFFFFFFFFFFFFFFFF
    info = np.iinfo(dtype)
    span = (1 << width) - 1
    k = n - 1 if delta else n
    r = rng.integers(0, span, k, dtype=np.uint64, endpoint=True) if width else np.zeros(k, np.uint64)
    if width:
        i, j = rng.choice(k, 2, replace=False)
        r[i], r[j] = 0, span
    if delta:
        lo = int(rng.integers(-(1 << 63), (1 << 63) - 1 - span, endpoint=True))  # the lowest signed residual
        first = np.uint64(int(rng.integers(0, 1 << 62)))
        steps = np.concatenate([[first], r + np.uint64(lo & M)])
        return np.cumsum(steps, dtype=np.uint64).view(np.int64)  # (wraps modulo 2^64)
    vmin = info.min if vmin is None else vmin
    vmax = info.max if vmax is None else vmax
    lo = int(rng.integers(vmin, vmax - span, endpoint=True))
    return (r.astype(np.int64) + np.int64(lo)).astype(dtype)
