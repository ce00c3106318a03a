"""Developer probe: packed typed columns, in one process and alternating, REPS
repeats after WARM warm-up rounds, each figure as median (min - max):

  config 2 (64 logs x 1 M records in 16 KiB segments)
    columns_to_host   clg_decode_logs_columns delivered to registered host memory (the existing
                      path), against
    packed_to_host    clg_decode_logs_columns_packed delivered to registered host memory: the host
                      clock around calls that end in a synchronise, the bytes each delivers, and
                      the packed call's kernel time by stat (decode_pipeline, decode_columns,
                      pack_columns; HIP events), and pack_columns once more with desc and bits in
                      device memory (the kernels off the link)
    unpack_host       clg_unpack_columns_host of every stream of that packed output, one thread,
                      on this machine's host: values/s and GB/s of output
  config 3 (PROBE_C3_LOGS logs of one PROBE_C3_REC-record epoch: random rng values, wide rows,
  payloads): the same two deliveries with the payload column (clg_decode_logs_columns_var against
  the packed call with var), bytes and wall time.

Writes profiles/pack_probe.json and prints it.  PROBE_SKIP_C3=1 leaves config 3 out (a profiler
run of the kernels)."""
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
from clonos_amd.engine import PACK_BLOCK, PACK_STREAM_FIELDS  # noqa: E402

WIDE = (("w_idx", 4), ("w_rc", 4), ("w_v1", 8), ("w_var_off", 4), ("w_var_len", 4), ("w_sub", 1), ("w_v0", 8))
NARROW = (("tag", 1), ("order", 1), ("timestamp", 8), ("rng", 4), ("buffer_built", 4))


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


def measure(eng, logs, ep, payloads, label):
    """The plain and the packed delivery of `logs` into registered host memory, alternating."""
    n = len(logs)
    h = np.array([lg.handle for lg in logs], np.uint32)
    ep = np.asarray(ep, np.int64)
    call_plain = _lib.lib.clg_decode_logs_columns_var if payloads else None
    # sizes: one sizes-only packed call gives every total
    sb = np.zeros((n + 1) * 5, np.uint64)
    wide, pk, pv = _lib.Columns(), _lib.Packed(), _lib.Payloads()
    wide.span_base = sb.ctypes.data
    st = _lib.lib.clg_decode_logs_columns_packed(eng.handle, h.ctypes.data, ep.ctypes.data, n, C.byref(wide),
                                                 C.byref(pv) if payloads else None, C.byref(pk))
    _lib.check(st)
    nr, ncls = int(wide.n_rec), [int(x) for x in wide.n_class]
    nw, nb, nbits = ncls[4], int(pk.blk_base[5]), int(pk.n_bits)
    nrows, nvar = int(pv.n_rows), int(pv.n_var)
    cnt = [nr] + ncls[:4]

    # the plain columns: every array in one registered region
    plain_sizes = [c * w for c, (_, w) in zip(cnt, NARROW)] + [nw * w for _, w in WIDE] + [nvar, 8 * (nrows + 1)]
    pc = Carver(plain_sizes)
    c = _lib.Columns()
    for i, (name, _) in enumerate(NARROW + WIDE):
        setattr(c, name, pc.ptr(i))
    c.cap_tag, c.cap_order, c.cap_timestamp, c.cap_rng, c.cap_buffer_built, c.cap_wide = *[max(x, 1) for x in cnt], max(nw, 1)
    sb_plain = np.zeros((n + 1) * 5, np.uint64)
    c.span_base, c.out_kind = sb_plain.ctypes.data, _lib.CLG_MEM_MAPPED
    p_plain = _lib.Payloads()
    p_plain.var, p_plain.pos, p_plain.cap_var, p_plain.cap_pos = pc.ptr(12), pc.ptr(13), max(nvar, 1), nrows + 1
    p_plain.out_kind = _lib.CLG_MEM_MAPPED

    # the packed form: desc, bits, the wide rows, the payload column
    packed_sizes = [32 * nb, nbits] + [nw * w for _, w in WIDE] + [nvar, 8 * (nrows + 1)]
    kc = Carver(packed_sizes)
    pk = _lib.Packed()
    pk.desc, pk.bits, pk.cap_desc, pk.cap_bits, pk.out_kind = kc.ptr(0), kc.ptr(1), nb, max(nbits, 16), _lib.CLG_MEM_MAPPED
    wide = _lib.Columns()
    for i, (name, _) in enumerate(WIDE):
        setattr(wide, name, kc.ptr(2 + i))
    wide.cap_wide, wide.span_base, wide.out_kind = max(nw, 1), sb.ctypes.data, _lib.CLG_MEM_MAPPED
    p_pack = _lib.Payloads()
    p_pack.var, p_pack.pos, p_pack.cap_var, p_pack.cap_pos = kc.ptr(9), kc.ptr(10), max(nvar, 1), nrows + 1
    p_pack.out_kind = _lib.CLG_MEM_MAPPED

    # the packed form once more with desc and bits in device memory: the pack kernels off the link
    ddesc = torch.empty(max(32 * nb, 16), dtype=torch.uint8, device="cuda")
    dbits = torch.empty(max(nbits, 16), dtype=torch.uint8, device="cuda")
    pk_dev = _lib.Packed()
    pk_dev.desc, pk_dev.bits, pk_dev.cap_desc, pk_dev.cap_bits = ddesc.data_ptr(), dbits.data_ptr(), nb, max(nbits, 16)
    pk_dev.out_kind = _lib.CLG_MEM_DEVICE
    wide_dev = _lib.Columns()  # (the wide rows sized, not delivered)

    stats = ("decode_pipeline", "decode_columns", "columns_small", "decode_payloads", "pack_columns")
    ms = {"plain": [], "packed": []}
    kern = {k: [] for k in stats}
    pack_dev = []
    for k in range(WARM + REPS):
        if k == WARM:
            ms = {"plain": [], "packed": []}
            kern = {name: [] for name in stats}
            pack_dev = []
        eng.kernel_stats_reset()
        _lib.check(_lib.lib.clg_decode_logs_columns_packed(eng.handle, h.ctypes.data, ep.ctypes.data, n, C.byref(wide_dev),
                                                           None, C.byref(pk_dev)))
        pack_dev.append(eng.kernel_stats()["pack_columns"]["ms"])
        eng.sync()
        t0 = time.perf_counter()
        if payloads:
            st = call_plain(eng.handle, h.ctypes.data, ep.ctypes.data, n, C.byref(c), C.byref(p_plain))
        else:
            st = _lib.lib.clg_decode_logs_columns(eng.handle, h.ctypes.data, ep.ctypes.data, n, C.byref(c))
        t1 = time.perf_counter()
        _lib.check(st)
        eng.kernel_stats_reset()
        t2 = time.perf_counter()
        st = _lib.lib.clg_decode_logs_columns_packed(eng.handle, h.ctypes.data, ep.ctypes.data, n, C.byref(wide),
                                                     C.byref(p_pack) if payloads else None, C.byref(pk))
        t3 = time.perf_counter()
        _lib.check(st)
        ks = eng.kernel_stats()
        for name in stats:
            kern[name].append(ks[name]["ms"] if name in ks else 0.0)
        ms["plain"].append((t1 - t0) * 1e3)
        ms["packed"].append((t3 - t2) * 1e3)

    # the two deliveries hold the same values: unpack the packed one on this host and compare
    desc = np.frombuffer(C.string_at(kc.ptr(0), 32 * nb), PACK_BLOCK).copy()
    bits = np.frombuffer(C.string_at(kc.ptr(1), nbits), np.uint8).copy() if nbits else np.zeros(0, np.uint8)
    good = _lib.Packed()
    good.desc, good.bits, good.cap_desc, good.cap_bits = desc.ctypes.data, bits.ctypes.data if nbits else None, nb, nbits
    for i in range(5):
        good.n_val[i] = pk.n_val[i]
    for i in range(6):
        good.blk_base[i] = pk.blk_base[i]
    good.n_bits = nbits
    unpack_s, out_bytes = [], 0
    outs = [np.empty(max(cnt[s], 1), dt) for s, (_, dt) in enumerate(PACK_STREAM_FIELDS)]
    for rep in range(3):
        t0 = time.perf_counter()
        for s in range(5):
            _lib.check(_lib.lib.clg_unpack_columns_host(C.byref(good), s, 0, cnt[s], outs[s].ctypes.data))
        unpack_s.append(time.perf_counter() - t0)
    for s, (name, w) in enumerate(NARROW):
        want = np.frombuffer(C.string_at(pc.ptr(s), cnt[s] * w), outs[s].dtype)
        assert (outs[s][:cnt[s]] == want).all(), name
        out_bytes += cnt[s] * w
    assert (sb == sb_plain).all()
    n_values = sum(cnt)
    side = sum(nw * w for _, w in WIDE) + 40 * (n + 1) + (nvar + 8 * (nrows + 1) if payloads else 0)
    plain_bytes, packed_bytes = out_bytes + side, 32 * nb + nbits + side
    widths = {name: sorted(set(int(x) for x in desc["width"][int(pk.blk_base[s]):int(pk.blk_base[s + 1])]))
              for s, (name, _) in enumerate(NARROW)}
    res = {
        "workload": label, "records": nr, "class_totals": ncls, "blocks": nb, "payload_rows": nrows, "payload_bytes": nvar,
        "widths_seen": widths,
        "plain_to_host_ms": spread(ms["plain"]), "packed_to_host_ms": spread(ms["packed"]),
        "plain_bytes_delivered": plain_bytes, "packed_bytes_delivered": packed_bytes,
        "narrow_bytes_plain": out_bytes, "narrow_bytes_packed": 32 * nb + nbits,
        "bytes_ratio": round(plain_bytes / packed_bytes, 3),
        "wall_ratio": round(float(np.median(ms["plain"]) / np.median(ms["packed"])), 3),
        "packed_call_kernel_ms": {name: spread(v) for name, v in kern.items() if any(v)},
        "pack_columns_device_output_ms": spread(pack_dev),
        "unpack_host_one_thread": {
            "seconds": spread(unpack_s), "values_per_s": round(n_values / float(np.median(unpack_s))),
            "output_GB_per_s": round(out_bytes / float(np.median(unpack_s)) / 1e9, 3)},
    }
    pc.release()
    kc.release()
    return res


def open_logs(eng, bufs, first):
    logs = []
    for v, b in enumerate(bufs):
        lg = eng.open_log(CausalLogID.main(first + v))
        lg.processUpstreamDelta(b.tobytes(), 0, 1)
        logs.append(lg)
    return logs


res = {"reps": REPS, "warmup_rounds": WARM,
       "note": ("wall: host clock around synchronous calls into host memory registered with clg_host_register, the plain "
                "and the packed call alternating in one process; kernel ms: HIP-event time of all kernels of the packed "
                "call under each stat; unpack: one thread on the GPU machine's host.")}
rng = np.random.default_rng(synth.SEED_CONFIG2)
bufs = [synth.config2_log(n_rec, rng)[0] for _ in range(n_logs)]
seg = 16384
c3 = None if os.environ.get("PROBE_SKIP_C3") else synth.config3_epoch(c3_rec, np.random.default_rng(3))[0]
pool = sum(int(b.size) // seg + 2 for b in bufs) + (0 if c3 is None else c3_logs * (int(c3.size) // seg + 2)) + 64
with Engine(segment_bytes=seg, pool_segments=pool, timing=True) as eng:
    logs = open_logs(eng, bufs, 0)
    res["config2"] = measure(eng, logs, np.ones(n_logs), False,
                             f"config 2: {n_logs} logs x {n_rec} records, {sum(int(b.size) for b in bufs)} bytes")
    if c3 is not None:
        logs3 = open_logs(eng, [c3] * c3_logs, 1000)
        res["config3"] = measure(eng, logs3, np.ones(c3_logs), True,
                                 f"config 3: {c3_logs} logs, each one epoch of {c3_rec} records ({int(c3.size)} bytes), "
                                 "with the payload column")

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "pack_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
