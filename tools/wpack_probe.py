"""Developer probe: packed wide rows, in one process and alternating, REPS repeats
after WARM warm-up rounds, each figure as median (min - max).  On config 3 (PROBE_C3_LOGS logs of one
PROBE_C3_REC-record epoch, with the payload column) and on config 2 (PROBE_LOGS logs x PROBE_REC
records, no wide rows), into host memory registered with clg_host_register:

  (a) plain     clg_decode_logs_columns[_var]: every column plain
  (b) packed    clg_decode_logs_columns_packed: the narrow columns packed, the wide rows and pos plain
  (c) wide      clg_decode_logs_columns_packed_wide: the wide rows packed by kind as well, no pos

the host clock around calls that end in a synchronise, the bytes each delivers by part, (c)'s kernel
time by stat, and pack_wide and pack_columns once more with their outputs in device memory (the
kernels off the link: pack_columns is pack_wide's yardstick).  (c)'s output is unpacked on this host
and held against (a)'s.

Writes profiles/wpack_probe.json and prints it."""
import ctypes as C
import json
import mmap
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = int(os.environ.get("PROBE_REPS", 10)), int(os.environ.get("PROBE_WARM", 3))
n_logs, n_rec = int(os.environ.get("PROBE_LOGS", 64)), int(os.environ.get("PROBE_REC", 1_000_000))
c3_logs, c3_rec = int(os.environ.get("PROBE_C3_LOGS", 16)), int(os.environ.get("PROBE_C3_REC", 250_000))

import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, synth  # noqa: E402
from clonos_amd.engine import PACK_BLOCK, PackedWide  # noqa: E402

WIDE = (("w_idx", 4, np.uint32), ("w_rc", 4, np.int32), ("w_v1", 8, np.int64), ("w_var_off", 4, np.uint32),
        ("w_var_len", 4, np.uint32), ("w_sub", 1, np.uint8), ("w_v0", 8, np.int64))
NARROW = (("tag", 1), ("order", 1), ("timestamp", 8), ("rng", 4), ("buffer_built", 4))
WS = _lib.WPACK_STREAMS


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def registered(nbytes):
    buf = np.frombuffer(mmap.mmap(-1, (nbytes + 4095) & ~4095), np.uint8)
    buf[:] = 0  # fault the pages in before they are pinned
    _lib.check(_lib.lib.clg_host_register(buf.ctypes.data, buf.size))
    return buf


class Carver:
    """Arrays carved out of one registered region, 256 bytes apart."""

    def __init__(self, sizes):
        self.at, total = [], 0
        for s in sizes:
            self.at.append(total)
            total = (total + max(s, 1) + 255) & ~255
        self.buf = registered(total + 4096)

    def ptr(self, i):
        return self.buf.ctypes.data + self.at[i]

    def release(self):
        _lib.lib.clg_host_unregister(self.buf.ctypes.data)


def packed_at(cls, desc, bits, nb, nbits, kind):
    p = cls()
    p.desc, p.bits, p.cap_desc, p.cap_bits, p.out_kind = desc, bits, nb, max(nbits, 16), kind
    return p


def measure(eng, logs, ep, payloads, label):
    n = len(logs)
    h = np.array([lg.handle for lg in logs], np.uint32)
    ep = np.asarray(ep, np.int64)
    args = (eng.handle, h.ctypes.data, ep.ctypes.data, n)
    lib = _lib.lib
    # every total from one sizes-only call
    sizes, pk, wpk, pv = _lib.Columns(), _lib.Packed(), _lib.PackedWideC(), _lib.Payloads()
    _lib.check(lib.clg_decode_logs_columns_packed_wide(*args, C.byref(sizes), C.byref(pv) if payloads else None,
                                                       C.byref(pk), C.byref(wpk)))
    nr, ncls = int(sizes.n_rec), [int(x) for x in sizes.n_class]
    nw, nb, nbits = ncls[4], int(pk.blk_base[5]), int(pk.n_bits)
    wnb, wnbits = int(wpk.blk_base[WS]), int(wpk.n_bits)
    nrows, nvar = int(pv.n_rows), int(pv.n_var)
    cnt = [nr] + ncls[:4]
    wide_sizes = [nw * w for _, w, _ in WIDE]

    # (a) the plain columns
    ac = Carver([c * w for c, (_, w) in zip(cnt, NARROW)] + wide_sizes + [nvar, 8 * (nrows + 1)])
    a_cols = _lib.Columns()
    for i, name in enumerate([x[0] for x in NARROW] + [x[0] for x in WIDE]):
        setattr(a_cols, name, ac.ptr(i))
    a_cols.cap_tag, a_cols.cap_order, a_cols.cap_timestamp, a_cols.cap_rng, a_cols.cap_buffer_built = [max(x, 1) for x in cnt]
    a_cols.cap_wide = max(nw, 1)
    sb_a = np.zeros((n + 1) * 5, np.uint64)
    a_cols.span_base, a_cols.out_kind = sb_a.ctypes.data, _lib.CLG_MEM_MAPPED
    a_pay = _lib.Payloads()
    a_pay.var, a_pay.pos, a_pay.cap_var, a_pay.cap_pos, a_pay.out_kind = ac.ptr(12), ac.ptr(13), max(nvar, 1), nrows + 1, _lib.CLG_MEM_MAPPED

    # (b) narrow packed; the wide rows, var and pos plain
    bc = Carver([32 * nb, nbits] + wide_sizes + [nvar, 8 * (nrows + 1)])
    b_pk = packed_at(_lib.Packed, bc.ptr(0), bc.ptr(1), nb, nbits, _lib.CLG_MEM_MAPPED)
    b_wide = _lib.Columns()
    for i, (name, _, _) in enumerate(WIDE):
        setattr(b_wide, name, bc.ptr(2 + i))
    sb_b = np.zeros((n + 1) * 5, np.uint64)
    b_wide.cap_wide, b_wide.span_base, b_wide.out_kind = max(nw, 1), sb_b.ctypes.data, _lib.CLG_MEM_MAPPED
    b_pay = _lib.Payloads()
    b_pay.var, b_pay.pos, b_pay.cap_var, b_pay.cap_pos, b_pay.out_kind = bc.ptr(9), bc.ptr(10), max(nvar, 1), nrows + 1, _lib.CLG_MEM_MAPPED

    # (c) narrow and wide packed; var without pos
    cc = Carver([32 * nb, nbits, 32 * wnb, wnbits, nvar])
    c_pk = packed_at(_lib.Packed, cc.ptr(0), cc.ptr(1), nb, nbits, _lib.CLG_MEM_MAPPED)
    c_wpk = packed_at(_lib.PackedWideC, cc.ptr(2), cc.ptr(3), wnb, wnbits, _lib.CLG_MEM_MAPPED)
    sb_c = np.zeros((n + 1) * 5, np.uint64)
    c_sizes = _lib.Columns()
    c_sizes.span_base, c_sizes.out_kind = sb_c.ctypes.data, _lib.CLG_MEM_MAPPED
    c_pay = _lib.Payloads()
    c_pay.var, c_pay.cap_var, c_pay.out_kind = cc.ptr(4), max(nvar, 1), _lib.CLG_MEM_MAPPED

    # (c) once more with the packed outputs in device memory: the pack kernels off the link
    dev = [torch.empty(max(x, 16), dtype=torch.uint8, device="cuda") for x in (32 * nb, nbits, 32 * wnb, wnbits)]
    d_pk = packed_at(_lib.Packed, dev[0].data_ptr(), dev[1].data_ptr(), nb, nbits, _lib.CLG_MEM_DEVICE)
    d_wpk = packed_at(_lib.PackedWideC, dev[2].data_ptr(), dev[3].data_ptr(), wnb, wnbits, _lib.CLG_MEM_DEVICE)
    d_sizes = _lib.Columns()

    stats = ("decode_pipeline", "decode_columns", "columns_small", "decode_payloads", "pack_columns", "pack_wide")
    ms = {k: [] for k in "abc"}
    kern = {k: [] for k in stats}
    dev_ms = {"pack_columns": [], "pack_wide": []}
    for k in range(WARM + REPS):
        if k == WARM:
            ms = {x: [] for x in "abc"}
            kern = {name: [] for name in stats}
            dev_ms = {"pack_columns": [], "pack_wide": []}
        eng.kernel_stats_reset()
        _lib.check(lib.clg_decode_logs_columns_packed_wide(*args, C.byref(d_sizes), None, C.byref(d_pk), C.byref(d_wpk)))
        ks = eng.kernel_stats()
        for name in dev_ms:
            dev_ms[name].append(ks[name]["ms"] if name in ks else 0.0)
        eng.sync()
        t0 = time.perf_counter()
        if payloads:
            st = lib.clg_decode_logs_columns_var(*args, C.byref(a_cols), C.byref(a_pay))
        else:
            st = lib.clg_decode_logs_columns(*args, C.byref(a_cols))
        t1 = time.perf_counter()
        _lib.check(st)
        t2 = time.perf_counter()
        st = lib.clg_decode_logs_columns_packed(*args, C.byref(b_wide), C.byref(b_pay) if payloads else None, C.byref(b_pk))
        t3 = time.perf_counter()
        _lib.check(st)
        eng.kernel_stats_reset()
        t4 = time.perf_counter()
        st = lib.clg_decode_logs_columns_packed_wide(*args, C.byref(c_sizes), C.byref(c_pay) if payloads else None,
                                                     C.byref(c_pk), C.byref(c_wpk))
        t5 = time.perf_counter()
        _lib.check(st)
        ks = eng.kernel_stats()
        for name in stats:
            kern[name].append(ks[name]["ms"] if name in ks else 0.0)
        ms["a"].append((t1 - t0) * 1e3), ms["b"].append((t3 - t2) * 1e3), ms["c"].append((t5 - t4) * 1e3)

    # (c) holds (a)'s values: the narrow bytes are (b)'s, the wide rows unpack to (a)'s, var is (a)'s
    assert C.string_at(cc.ptr(0), 32 * nb) == C.string_at(bc.ptr(0), 32 * nb) and C.string_at(cc.ptr(1), nbits) == C.string_at(bc.ptr(1), nbits)
    wide = PackedWide(np.frombuffer(C.string_at(cc.ptr(2), 32 * wnb), PACK_BLOCK).copy(),
                      np.frombuffer(C.string_at(cc.ptr(3), wnbits), np.uint8).copy(), c_wpk.n_val, c_wpk.blk_base)
    t0 = time.perf_counter()
    back = wide.unpack()
    unpack_s = time.perf_counter() - t0
    for i, (name, w, dt) in enumerate(WIDE):
        assert (back[name] == np.frombuffer(C.string_at(ac.ptr(5 + i), nw * w), dt)).all(), name
    if payloads:
        assert C.string_at(cc.ptr(4), nvar) == C.string_at(ac.ptr(12), nvar)
        pos = np.frombuffer(C.string_at(ac.ptr(13), 8 * (nrows + 1)), np.uint64)
        assert (np.concatenate([[0], np.cumsum(back["w_var_len"], dtype=np.uint64)]) == pos).all()
    assert (sb_a == sb_c).all() and (sb_b == sb_c).all()

    narrow_plain = sum(c * w for c, (_, w) in zip(cnt, NARROW))
    wide_plain, pos_bytes = sum(wide_sizes), 8 * (nrows + 1) if payloads else 0
    var_bytes, base_bytes = (nvar if payloads else 0), 40 * (n + 1)
    parts = {
        "a_plain": {"narrow": narrow_plain, "wide_rows": wide_plain, "pos": pos_bytes, "var": var_bytes, "span_base": base_bytes},
        "b_packed": {"narrow": 32 * nb + nbits, "wide_rows": wide_plain, "pos": pos_bytes, "var": var_bytes, "span_base": base_bytes},
        "c_packed_wide": {"narrow": 32 * nb + nbits, "wide_rows": 32 * wnb + wnbits, "pos": 0, "var": var_bytes, "span_base": base_bytes},
    }
    tot = {k: sum(v.values()) for k, v in parts.items()}
    kinds = [int(c_wpk.n_val[2 + 6 * t]) for t in range(4)]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {
        "workload": label, "records": nr, "class_totals": ncls, "wide_rows_by_kind": kinds,
        "narrow_blocks": nb, "wide_blocks": wnb, "payload_bytes": nvar,
        "delivered_bytes_by_part": parts, "delivered_bytes": tot,
        "wide_rows_and_pos_c_over_b": round((32 * wnb + wnbits) / max(wide_plain + pos_bytes, 1), 4),
        "wide_rows_c_over_plain_arrays": round((32 * wnb + wnbits) / max(wide_plain, 1), 4),
        "bytes_ratio_b_over_c": round(tot["b_packed"] / tot["c_packed_wide"], 3),
        "bytes_ratio_a_over_c": round(tot["a_plain"] / tot["c_packed_wide"], 3),
        "wall_ms": {"a_plain": spread(ms["a"]), "b_packed": spread(ms["b"]), "c_packed_wide": spread(ms["c"])},
        "wall_ratio_b_over_c": round(med["b"] / med["c"], 3), "wall_ratio_a_over_c": round(med["a"] / med["c"], 3),
        "c_call_kernel_ms": {name: spread(v) for name, v in kern.items() if any(v)},
        "device_output_kernel_ms": {name: spread(v) for name, v in dev_ms.items()},
        "pack_wide_over_pack_columns_device_outputs": round(float(np.median(dev_ms["pack_wide"])) /
                                                            max(float(np.median(dev_ms["pack_columns"])), 1e-9), 3),
        "unpack_wide_host_one_thread_s": round(unpack_s, 4),
    }
    ac.release(), bc.release(), cc.release()
    return res


def open_logs(eng, bufs, first):
    logs = []
    for v, b in enumerate(bufs):
        lg = eng.open_log(CausalLogID.main(first + v))
        lg.processUpstreamDelta(b.tobytes(), 0, 1)
        logs.append(lg)
    return logs


res = {"reps": REPS, "warmup_rounds": WARM,
       "note": ("wall: host clock around synchronous calls into host memory registered with clg_host_register, the three "
                "calls alternating in one process; kernel ms: HIP-event time of all kernels of the call under each stat; "
                "device_output_kernel_ms: the packed-wide call without payloads, desc and bits of both packs in device memory.")}
rng = np.random.default_rng(synth.SEED_CONFIG2)
bufs = [synth.config2_log(n_rec, rng)[0] for _ in range(n_logs)]
seg = 16384
c3 = synth.config3_epoch(c3_rec, np.random.default_rng(3))[0]
pool = sum(int(b.size) // seg + 2 for b in bufs) + c3_logs * (int(c3.size) // seg + 2) + 64
with Engine(segment_bytes=seg, pool_segments=pool, timing=True) as eng:
    logs3 = open_logs(eng, [c3] * c3_logs, 1000)
    res["config3"] = measure(eng, logs3, np.ones(c3_logs), True,
                             f"config 3: {c3_logs} logs, each one epoch of {c3_rec} records ({int(c3.size)} bytes), "
                             "with the payload column")
    logs = open_logs(eng, bufs, 0)
    res["config2"] = measure(eng, logs, np.ones(n_logs), False,
                             f"config 2: {n_logs} logs x {n_rec} records, {sum(int(b.size) for b in bufs)} bytes")

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "wpack_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
