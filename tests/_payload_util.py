"""Shared by the payload-column GPU tests: the expected column by plain numpy slicing of the span
bytes, uploads, and var / pos buffers with guard bytes either side in device, registered-host
and plain host memory."""
import ctypes
import mmap

import numpy as np

GUARD = 64   # guard bytes either side of var and of pos (keeps both 64-byte aligned)
FILL = 0xA5
NO_ROW = 0xFFFFFFFFFFFFFFFF


def expected(spans, wo, wl, rb):
    """(var, pos) by slicing: spans is a list of uint8 arrays, row k of span s (rb[s] <= k < rb[s + 1])
    contributes spans[s][wo[k] : wo[k] + wl[k]].  Vectorised per span; every row must lie inside its
    span (asserted)."""
    wo, wl = np.asarray(wo, np.int64), np.asarray(wl, np.int64)
    pos = np.concatenate([[0], np.cumsum(wl)]).astype(np.uint64)
    parts = []
    for s, span in enumerate(spans):
        a, b = int(rb[s]), int(rb[s + 1])
        o, l = wo[a:b], wl[a:b]
        assert ((o + l) <= len(span)).all()
        if int(l.sum()) == 0:
            continue
        start = np.repeat(o, l)
        within = np.arange(int(l.sum())) - np.repeat(np.cumsum(l) - l, l)
        parts.append(np.asarray(span, np.uint8)[start + within])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), pos


def upload(a):
    """The array's bytes in device memory (a tests/_devbuf.DeviceBuf; at least one byte)."""
    from _devbuf import DeviceBuf
    a = np.ascontiguousarray(a)
    b = DeviceBuf(max(a.nbytes, 1))
    if a.nbytes:
        assert b.hip.hipMemcpy(b.p, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes), 1) == 0
    return b


class GuardedPayloads:
    """A clg_payloads whose var (cap_var bytes) and pos (cap_pos entries) have GUARD bytes of FILL
    either side, in device memory, registered host memory (CLG_MEM_MAPPED) or plain host memory."""

    def __init__(self, kind, cap_var, cap_pos):
        from clonos_amd import _lib
        self.kind, self._lib = kind, _lib
        self.p = _lib.Payloads()
        self.p.out_kind = {"device": _lib.CLG_MEM_DEVICE, "mapped": _lib.CLG_MEM_MAPPED, "host": _lib.CLG_MEM_HOST}[kind]
        self.p.cap_var, self.p.cap_pos = cap_var, cap_pos
        sizes = {"var": 2 * GUARD + cap_var, "pos": 2 * GUARD + 8 * cap_pos}
        self.bufs = {}
        if kind == "mapped":
            total = sum((s + 63) & ~63 for s in sizes.values())
            self.region = np.frombuffer(mmap.mmap(-1, (total + 4095) & ~4095), np.uint8)
            self.region[:] = FILL
            _lib.check(_lib.lib.clg_host_register(self.region.ctypes.data, self.region.size))
        at = 0
        for name in ("var", "pos"):
            if kind == "device":
                from _devbuf import DeviceBuf
                b = DeviceBuf(sizes[name], fill=FILL)
                ptr = b.p.value
            elif kind == "mapped":
                b = self.region[at:at + sizes[name]]
                at += (sizes[name] + 63) & ~63
                ptr = b.ctypes.data
            else:
                b = np.full(sizes[name], FILL, np.uint8)
                ptr = b.ctypes.data
            self.bufs[name] = b
            setattr(self.p, name, ptr + GUARD)

    def raw(self, name):
        b = self.bufs[name]
        return b.host() if self.kind == "device" else np.array(b)

    def guards_intact(self):
        return all((r[:GUARD] == FILL).all() and (r[r.size - GUARD:] == FILL).all()
                   for r in (self.raw("var"), self.raw("pos")))

    def untouched(self):
        return bool((self.raw("var") == FILL).all() and (self.raw("pos") == FILL).all())

    def result(self):
        """(var[:n_var], pos[:n_rows + 1]) the call filled (copies)."""
        nv, nr = int(self.p.n_var), int(self.p.n_rows)
        return (self.raw("var")[GUARD:GUARD + nv].copy(),
                self.raw("pos")[GUARD:GUARD + 8 * (nr + 1)].copy().view(np.uint64))

    def after_result(self):
        """The bytes between the results' ends and the closing guards (capacity above the totals)."""
        nv, nr = int(self.p.n_var), int(self.p.n_rows)
        v, q = self.raw("var"), self.raw("pos")
        return v[GUARD + nv:], q[GUARD + 8 * (nr + 1):]

    def free(self):
        if self.kind == "device":
            for b in self.bufs.values():
                b.free()
        elif self.kind == "mapped":
            self._lib.lib.clg_host_unregister(self.region.ctypes.data)
        self.bufs = {}
