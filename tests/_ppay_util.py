"""Shared by the packed-payload-column tests: an independent numpy packer and unpacker written from
the format's description (include/clonos_engine.h, "the packed payload column"; it shares no code
with clonos_amd/csrc/ppay.h: anchors through np.unique, lcps by array comparison, the LCP blocks
through tests/_pack_util.py's bit matrix), the scene builders, and guarded buffers in device,
registered-host and plain host memory."""
import ctypes
import mmap

import numpy as np

from _pack_util import DESC, pack_block

TILE = 1024
GUARD = 64   # guard bytes either side of every buffer (keeps them 64-byte aligned)
FILL = 0xA5
NO_ROW = 0xFFFFFFFFFFFFFFFF
WAVE_ROW = 64      # kPayWaveRow: rows of at least this many bytes are handled by a wave
SLOTS = 2048       # the device's anchor table
HASH_MUL, HASH_SHIFT = 0x9E3779B1, 21


def table_hash(length):
    """The device table's slot of a length (clonos_amd/csrc/ppay.h ppay_hash)."""
    return ((int(length) * HASH_MUL) & 0xFFFFFFFF) >> HASH_SHIFT


# ---- the format, in numpy ----------------------------------------------------------------------

def anchors_of(lens):
    """anchor(k) for every row: the lowest row of k's tile with k's length."""
    lens = np.asarray(lens, np.int64)
    a = np.empty(lens.size, np.int64)
    for t0 in range(0, lens.size, TILE):
        _, first, inv = np.unique(lens[t0:t0 + TILE], return_index=True, return_inverse=True)
        a[t0:t0 + TILE] = t0 + first[inv.reshape(-1)]
    return a


def lcps_of(var, pos):
    """The maximal lcp of every row against its anchor (0 for an anchor)."""
    var, pos = np.asarray(var, np.uint8), np.asarray(pos, np.uint64).astype(np.int64)
    lens = np.diff(pos)
    anc = anchors_of(lens)
    lcp = np.zeros(lens.size, np.int64)
    for k in np.nonzero(anc != np.arange(lens.size))[0]:
        n = int(lens[k])
        ne = np.nonzero(var[pos[k]:pos[k] + n] != var[pos[anc[k]]:pos[anc[k]] + n])[0]
        lcp[k] = int(ne[0]) if ne.size else n
    return lcp, anc


def pack_numpy(var, pos, lcp=None):
    """(desc rows, bits, tail) of the column; lcp: other (non-maximal) lcps to emit."""
    var, pos = np.asarray(var, np.uint8), np.asarray(pos, np.uint64).astype(np.int64)
    if lcp is None:
        lcp, _ = lcps_of(var, pos)
    lcp = np.asarray(lcp, np.int64)
    rows, chunks, at = [], [], 0
    for t0 in range(0, lcp.size, TILE):
        blk = lcp[t0:t0 + TILE].astype(np.uint32)
        ref, first, width, payload = pack_block(blk, False)
        rows.append((ref, first, at, width, blk.size))
        chunks.append(payload)
        at += len(payload)
    n_var = int(pos[-1]) if pos.size else 0
    keep = np.ones(n_var, bool)
    if lcp.size and int(lcp.sum()):
        start = np.repeat(pos[:-1], lcp)
        within = np.arange(int(lcp.sum())) - np.repeat(np.cumsum(lcp) - lcp, lcp)
        keep[start + within] = False
    desc = np.array(rows, DESC) if rows else np.zeros(0, DESC)
    return desc, np.frombuffer(b"".join(chunks), np.uint8), var[:n_var][keep]


def decode_lcps(desc, bits):
    out = []
    for d in desc:
        n, w = int(d["count"]), int(d["width"])
        if w == 0:
            out.append(np.full(n, int(d["ref"]), np.int64))
            continue
        raw = np.asarray(bits, np.uint8)[int(d["pos"]):int(d["pos"]) + 16 * ((n * w + 127) // 128)]
        b = np.unpackbits(raw, bitorder="little")[:n * w].reshape(n, w).astype(np.uint64)
        out.append(int(d["ref"]) + (b << np.arange(w, dtype=np.uint64)).sum(axis=1).astype(np.int64))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def unpack_numpy(desc, bits, tail, pos):
    """var of a well-formed packed column: row k is tail_anchor(k)[:lcp_k] + tail_k."""
    pos = np.asarray(pos, np.uint64).astype(np.int64)
    lens = np.diff(pos)
    lcp = decode_lcps(desc, bits)
    anc = anchors_of(lens)
    toff = np.concatenate([[0], np.cumsum(lens - lcp)])
    tail = np.asarray(tail, np.uint8)
    var = np.empty(int(pos[-1]) if pos.size else 0, np.uint8)
    for k in range(lens.size):
        c, n = int(lcp[k]), int(lens[k])
        var[pos[k]:pos[k] + c] = tail[toff[anc[k]]:toff[anc[k]] + c]
        var[pos[k] + c:pos[k] + n] = tail[toff[k]:toff[k] + n - c]
    return var


def assert_packed_equals_numpy(packed, var, pos):
    desc, bits, tail = pack_numpy(var, pos)
    got = np.asarray(packed.desc)
    assert got.size == desc.size
    for f in DESC.names:
        assert (got[f] == desc[f]).all(), f
    assert np.asarray(packed.bits).tobytes() == bits.tobytes()
    assert np.asarray(packed.tail).tobytes() == tail.tobytes()
    assert packed.n_rows == len(pos) - 1 and packed.n_var == int(pos[-1])


def assert_same_packed(a, b):
    assert (a.n_rows, a.n_var) == (b.n_rows, b.n_var)
    for f in ("desc", "bits", "tail"):
        assert np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes(), f


# ---- scenes ------------------------------------------------------------------------------------

def column(rows):
    """(var, pos) of a list of byte strings."""
    pos = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    return np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).copy(), pos


def payload_column_of(spans):
    """The payload column of encoded spans: the oracle's batch, its columns on the CPU, the
    payload gather on the CPU."""
    from _columns_util import oracle_batch
    from clonos_amd import columnize_host, gather_payloads_host
    c = columnize_host(oracle_batch(spans))
    data = np.concatenate([np.frombuffer(bytes(s), np.uint8) for s in spans] + [np.zeros(0, np.uint8)])
    offs = np.concatenate([[0], np.cumsum([len(s) for s in spans])]).astype(np.uint64)
    return gather_payloads_host(data, offs[:-1], np.diff(offs), c.w_var_off, c.w_var_len, c.span_base[:, 4])


_CACHE = {}


def config3_column():
    """The payload column of synth.config3_epoch(3000, default_rng(0x9AC)), computed once."""
    if "config3" not in _CACHE:
        from clonos_amd import synth
        _CACHE["config3"] = payload_column_of([bytes(synth.config3_epoch(3000, np.random.default_rng(0x9AC))[0])])
    return _CACHE["config3"]


def random_log_column():
    if "random_log" not in _CACHE:
        from clonos_amd import synth
        _CACHE["random_log"] = payload_column_of([synth.random_log(1500, np.random.default_rng(0x9AD), allow_serializable=True)])
    return _CACHE["random_log"]


def seeded_rows(rng, n, lens, alphabet=4, share=0.7):
    """n rows with lengths drawn from `lens`; a row copies a prefix of an earlier row of its length
    with probability `share`, so that lcps of every size appear."""
    rows, by_len = [], {}
    for _ in range(n):
        L = int(rng.choice(lens))
        r = rng.integers(0, alphabet, L, dtype=np.uint8)
        if L in by_len and rng.random() < share:
            c = int(rng.integers(0, L + 1))
            r[:c] = by_len[L][:c]
        by_len.setdefault(L, r)
        rows.append(r.tobytes())
    return rows


def colliding_lengths(n=TILE, limit=3000):
    """n distinct lengths below `limit`, those that share a slot of the device's table first."""
    by_slot = {}
    for L in range(limit):
        by_slot.setdefault(table_hash(L), []).append(L)
    crowded = sorted(by_slot.values(), key=lambda v: (-len(v), v[0]))
    out = [L for v in crowded for L in v][:n]
    assert len(set(out)) == n and len({table_hash(L) for L in out}) < n
    return out


# ---- guarded buffers ---------------------------------------------------------------------------

class Guarded:
    """Named byte buffers with GUARD bytes of FILL either side, in device memory ("device"),
    registered host memory ("mapped") or plain host memory ("host").  ptr(name) is the address
    inside the guards; put(name, bytes) fills from the start."""

    def __init__(self, kind, sizes):
        from clonos_amd import _lib
        self.kind, self._lib, self.sizes = kind, _lib, dict(sizes)
        self.mem_kind = {"device": _lib.CLG_MEM_DEVICE, "mapped": _lib.CLG_MEM_MAPPED, "host": _lib.CLG_MEM_HOST}[kind]
        full = {k: 2 * GUARD + ((s + 15) & ~15) for k, s in self.sizes.items()}
        self.bufs, self._ptr = {}, {}
        if kind == "mapped":
            total = sum((s + 63) & ~63 for s in full.values())
            self.region = np.frombuffer(mmap.mmap(-1, (total + 4095) & ~4095), np.uint8)
            self.region[:] = FILL
            _lib.check(_lib.lib.clg_host_register(self.region.ctypes.data, self.region.size))
        at = 0
        for name, size in full.items():
            if kind == "device":
                from _devbuf import DeviceBuf
                b = DeviceBuf(size, fill=FILL)
                p = b.p.value
            elif kind == "mapped":
                b = self.region[at:at + size]
                at += (size + 63) & ~63
                p = b.ctypes.data
            else:
                b = np.full(size + 64, FILL, np.uint8)
                b = b[(-b.ctypes.data) % 64:][:size]
                p = b.ctypes.data
            self.bufs[name], self._ptr[name] = b, p + GUARD

    def ptr(self, name):
        return self._ptr[name]

    def put(self, name, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert data.size <= self.sizes[name]
        if not data.size:
            return
        if self.kind == "device":
            b = self.bufs[name]
            assert b.hip.hipMemcpy(ctypes.c_void_p(self._ptr[name]), ctypes.c_void_p(data.ctypes.data),
                                   ctypes.c_size_t(data.size), 1) == 0
        else:
            self.bufs[name][GUARD:GUARD + data.size] = data

    def raw(self, name):
        b = self.bufs[name]
        return b.host() if self.kind == "device" else np.array(b)

    def get(self, name, n):
        return self.raw(name)[GUARD:GUARD + n].copy()

    def intact_outside(self, name, n):
        """Everything but the first n bytes inside the guards still holds FILL."""
        r = self.raw(name)
        return bool((r[:GUARD] == FILL).all() and (r[GUARD + n:] == FILL).all())

    def untouched(self, *names):
        return all(bool((self.raw(n) == FILL).all()) for n in (names or self.bufs))

    def free(self):
        if self.kind == "device":
            for b in self.bufs.values():
                b.free()
        elif self.kind == "mapped":
            self._lib.lib.clg_host_unregister(self.region.ctypes.data)
        self.bufs = {}
