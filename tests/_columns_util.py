"""Shared by the typed-columns tests: the oracle's decode of spans as one DecodedBatch, seeded
hand-made batches, and column buffers with guard bytes either side in device, registered-host and
plain host memory."""
import mmap

import numpy as np

import _oracle as O

KEYS = ("off", "tag", "v0", "w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub")
DTYPES = (np.uint32, np.uint8, np.int64, np.uint32, np.int32, np.int64, np.uint32, np.uint32, np.uint8)
# clg_columns' arrays: name, dtype, the capacity field, the class whose total it holds (None: n_rec)
COLS = (("tag", np.uint8, "cap_tag", None), ("order", np.int8, "cap_order", 0),
        ("timestamp", np.int64, "cap_timestamp", 1), ("rng", np.int32, "cap_rng", 2),
        ("buffer_built", np.int32, "cap_buffer_built", 3), ("w_idx", np.uint32, "cap_wide", 4),
        ("w_rc", np.int32, "cap_wide", 4), ("w_v1", np.int64, "cap_wide", 4), ("w_var_off", np.uint32, "cap_wide", 4),
        ("w_var_len", np.uint32, "cap_wide", 4), ("w_sub", np.uint8, "cap_wide", 4), ("w_v0", np.int64, "cap_wide", 4))
GUARD = 64   # guard bytes either side of every column (keeps every column 64-byte aligned)
FILL = 0xA5


def oracle_batch(spans, allow_errors=False):
    """The oracle's decode of each span as one DecodedBatch (w_idx global, var offsets
    span-relative).  allow_errors: a span with a decode error contributes its records before the
    error; returns (batch, first error as (status, span, off, tag) or None)."""
    from clonos_amd import DecodedBatch
    parts, base, err = [], [0], None
    for s, b in enumerate(spans):
        st, r, eo, et = O.decode(bytes(b))
        if st != 0:
            assert allow_errors, (s, st)
            if err is None:
                err = (st, s, eo, et)
        r = dict(r)
        r["w_idx"] = (r["w_idx"].astype(np.uint64) + base[-1]).astype(np.uint32)
        parts.append(r)
        base.append(base[-1] + len(r["tag"]))
    cat = [np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dt) for k, dt in zip(KEYS, DTYPES)]
    batch = DecodedBatch(*cat, np.array(base, np.uint64), [np.frombuffer(bytes(b), np.uint8) for b in spans])
    return (batch, err) if allow_errors else batch


def made_batch(tag, rng, base=None):
    """A hand-made decoded batch over the given tags: v0 as the decode leaves it (the field's own
    width, sign-extended), a seeded side row per wide record."""
    from clonos_amd import DecodedBatch
    tag = np.asarray(tag, np.uint8)
    n = tag.size
    v0 = rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
    v0[tag == 0] = rng.integers(-128, 128, int((tag == 0).sum()))
    m32 = (tag == 2) | (tag == 7)
    v0[m32] = rng.integers(-(1 << 31), 1 << 31, int(m32.sum()))
    w_idx = np.nonzero((tag >= 3) & (tag <= 6))[0].astype(np.uint32)
    nw = w_idx.size
    return DecodedBatch(np.zeros(n, np.uint32), tag, v0, w_idx, rng.integers(0, 1 << 20, nw).astype(np.int32),
                        rng.integers(0, 1 << 45, nw, dtype=np.int64), rng.integers(0, 1 << 30, nw).astype(np.uint32),
                        rng.integers(0, 100, nw).astype(np.uint32), rng.integers(0, 256, nw).astype(np.uint8),
                        np.array([0, n] if base is None else base, np.uint64))


def assert_columns_equal(got, want):
    for name, dt, _, _ in COLS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == dt and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        assert (a == b).all(), name
    assert (np.asarray(got.span_base) == np.asarray(want.span_base)).all()


class GuardedColumns:
    """A clg_columns whose every array has GUARD bytes of FILL either side, in device memory
    (tests/_devbuf.DeviceBuf), registered host memory (CLG_MEM_MAPPED) or plain host memory.
    caps: elements per array name."""

    def __init__(self, kind, caps, n_spans):
        from clonos_amd import _lib
        self.kind, self.caps, self._lib = kind, dict(caps), _lib
        self.c = _lib.Columns()
        self.bufs = {}
        self.base = np.full((n_spans + 1) * 5, 0xFFFFFFFFFFFFFFFF, np.uint64)
        self.c.span_base = self.base.ctypes.data
        self.c.out_kind = {"device": _lib.CLG_MEM_DEVICE, "mapped": _lib.CLG_MEM_MAPPED, "host": _lib.CLG_MEM_HOST}[kind]
        sizes = {name: 2 * GUARD + self.caps[name] * np.dtype(dt).itemsize for name, dt, _, _ in COLS}
        if kind == "mapped":  # one registered mapping, the columns carved from it at 64-byte steps
            total = sum((s + 63) & ~63 for s in sizes.values())
            self.region = np.frombuffer(mmap.mmap(-1, (total + 4095) & ~4095), np.uint8)
            self.region[:] = FILL
            _lib.check(_lib.lib.clg_host_register(self.region.ctypes.data, self.region.size))
        at = 0
        for name, dt, capf, _ in COLS:
            if kind == "device":
                from _devbuf import DeviceBuf
                b = DeviceBuf(sizes[name], fill=FILL)
                p = b.p.value
            elif kind == "mapped":
                b = self.region[at:at + sizes[name]]
                at += (sizes[name] + 63) & ~63
                p = b.ctypes.data
            else:
                b = np.full(sizes[name], FILL, np.uint8)
                p = b.ctypes.data
            self.bufs[name] = b
            setattr(self.c, name, p + GUARD)
            if capf != "cap_wide":
                setattr(self.c, capf, self.caps[name])
        self.c.cap_wide = min(self.caps[name] for name, _, capf, _ in COLS if capf == "cap_wide")

    def raw(self, name):
        b = self.bufs[name]
        return b.host() if self.kind == "device" else np.array(b)

    def guards_intact(self):
        for name, _, _, _ in COLS:
            r = self.raw(name)
            if not ((r[:GUARD] == FILL).all() and (r[r.size - GUARD:] == FILL).all()):
                return False
        return True

    def untouched(self):
        return all((self.raw(name) == FILL).all() for name, _, _, _ in COLS)

    def result(self):
        """The columns the call filled, as a DecodedColumns (copies)."""
        from clonos_amd import DecodedColumns
        n = [int(x) for x in self.c.n_class]
        arrs = []
        for name, dt, _, cls in COLS:
            k = int(self.c.n_rec) if cls is None else n[cls]
            r = self.raw(name)
            arrs.append(r[GUARD:GUARD + k * np.dtype(dt).itemsize].copy().view(dt))
        return DecodedColumns(*arrs, self.base.copy())

    def free(self):
        if self.kind == "device":
            for b in self.bufs.values():
                b.free()
        elif self.kind == "mapped":
            self._lib.lib.clg_host_unregister(self.region.ctypes.data)
        self.bufs = {}


def exact_caps(n, n_class):
    return {name: (n if cls is None else int(n_class[cls])) for name, _, _, cls in COLS}


def to_device(batch):
    """The batch's arrays uploaded (torch tensors, kept by the caller) and their clg_decoded."""
    import torch
    from clonos_amd import _lib
    keep = {}
    d = _lib.Decoded()
    for k, dt in zip(KEYS, DTYPES):
        if k == "off":
            continue
        a = np.ascontiguousarray(getattr(batch, k), dt)
        t = torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0") if a.size else None
        keep[k] = t
        setattr(d, k, t.data_ptr() if t is not None else None)
    torch.cuda.synchronize()
    d.n_rec, d.n_wide, d.out_kind = batch.n_rec, len(batch.w_idx), _lib.CLG_MEM_DEVICE
    d.cap, d.wcap = d.n_rec, d.n_wide
    return d, keep
