"""Developer probe: packed typed columns back into an engine, in one process and
alternating, REPS repeats after WARM warm-up rounds, each figure as median (min - max).  For
config 2 (64 logs x 1 M records in 16 KiB segments) and config 3 (PROBE_C3_LOGS logs of one
PROBE_C3_REC-record epoch with payloads), the logs' packed columns (host arrays, as a standby
receives them) are restored into fresh epochs of destination logs:

  (a) host_unpack_append   PackedColumns.unpack() on one host thread, then
                           Engine.append_columns(plain host columns): the path the parent commit has
  (b) packed_append        Engine.append_columns(packed host input): clg_append_columns_packed
  (c) unpack_device        clg_unpack_columns with desc and bits in device memory and device outputs

Wall time is the host clock around synchronous calls; kernel ms is the HIP-event time of the kernels
under each stat.  After the last round the destination logs' digests are checked against the
sources'.  Writes profiles/unpack_probe.json and prints it.  PROBE_TRACE=1: config 2 only, (c)
beside a clg_decode_logs_columns into device memory (k_col_write writes the same plain bytes), for
a kernel trace; nothing is written."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = int(os.environ.get("PROBE_REPS", 10)), int(os.environ.get("PROBE_WARM", 3))
n_logs, n_rec = int(os.environ.get("PROBE_LOGS", 64)), int(os.environ.get("PROBE_REC", 1_000_000))
c3_logs, c3_rec = int(os.environ.get("PROBE_C3_LOGS", 16)), int(os.environ.get("PROBE_C3_REC", 250_000))
TRACE = os.environ.get("PROBE_TRACE") == "1"

import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, synth  # noqa: E402
from clonos_amd.engine import PACK_STREAM_FIELDS  # noqa: E402

ELEM = (1, 1, 8, 4, 4)
CAPS = ("cap_tag", "cap_order", "cap_timestamp", "cap_rng", "cap_buffer_built")


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def device_unpack_args(packed):
    """(clg_packed, clg_columns, keep) with every array in device memory."""
    desc = torch.from_numpy(np.ascontiguousarray(packed.desc).view(np.uint8).copy()).cuda()
    bits = torch.from_numpy(np.ascontiguousarray(packed.bits).copy()).cuda() if packed.bits.size else torch.empty(16, dtype=torch.uint8, device="cuda")
    p = packed._struct()
    p.desc, p.bits, p.out_kind = desc.data_ptr(), bits.data_ptr(), _lib.CLG_MEM_DEVICE
    outs = [torch.empty(max(n, 1) * el, dtype=torch.uint8, device="cuda") for n, el in zip(packed.n_val, ELEM)]
    c = _lib.Columns()
    for (name, _), o, n, cap in zip(PACK_STREAM_FIELDS, outs, packed.n_val, CAPS):
        setattr(c, name, o.data_ptr())
        setattr(c, cap, max(n, 1))
    c.out_kind = _lib.CLG_MEM_DEVICE
    return p, c, (desc, bits, outs)


def measure(eng, src, dst_a, dst_b, label):
    n = len(src)
    packed = eng.decode_logs_columns(src, [1] * n, packed=True, payloads=True)
    plain = packed.unpack()
    p_dev, c_dev, keep = device_unpack_args(packed)
    bad = _lib.UnpackBad()
    names = ("unpack_columns", "encode_columns", "append_columns_scatter")
    wall = {"a": [], "a_unpack": [], "b": [], "c": []}
    kern = {"a": {k: [] for k in names}, "b": {k: [] for k in names}, "c": []}
    for k in range(WARM + REPS):
        if k == WARM:
            wall = {key: [] for key in wall}
            kern = {"a": {x: [] for x in names}, "b": {x: [] for x in names}, "c": []}
        ep = [k + 1] * n
        eng.sync()
        eng.kernel_stats_reset()
        t0 = time.perf_counter()
        cols = packed.unpack()
        t1 = time.perf_counter()
        eng.append_columns(dst_a, ep, cols)
        t2 = time.perf_counter()
        ks = eng.kernel_stats()
        for x in names:
            kern["a"][x].append(ks[x]["ms"] if x in ks else 0.0)
        eng.kernel_stats_reset()
        t3 = time.perf_counter()
        eng.append_columns(dst_b, ep, packed)
        t4 = time.perf_counter()
        ks = eng.kernel_stats()
        for x in names:
            kern["b"][x].append(ks[x]["ms"] if x in ks else 0.0)
        eng.kernel_stats_reset()
        t5 = time.perf_counter()
        _lib.check(eng.unpack_columns_raw(p_dev, c_dev, bad))
        t6 = time.perf_counter()
        kern["c"].append(eng.kernel_stats()["unpack_columns"]["ms"])
        wall["a"].append((t2 - t0) * 1e3), wall["a_unpack"].append((t1 - t0) * 1e3)
        wall["b"].append((t4 - t3) * 1e3), wall["c"].append((t6 - t5) * 1e3)

    # both destinations hold the sources' bytes in the last epoch, and (c) wrote the plain columns
    last = [WARM + REPS] * n
    hs, ha, hb = ([lg.handle for lg in logs] for logs in (src, dst_a, dst_b))
    ds, da, db = eng.digest_logs(hs, [1] * n), eng.digest_logs(ha, last), eng.digest_logs(hb, last)
    for d in (da, db):
        assert (d["hash"] == ds["hash"]).all() and (d["len"] == ds["len"]).all()
    for (name, dt), o, cnt in zip(PACK_STREAM_FIELDS, keep[2], packed.n_val):
        assert (o.cpu().numpy().view(dt)[:cnt] == getattr(plain, name)).all(), name
    narrow_plain = sum(cnt * el for cnt, el in zip(packed.n_val, ELEM))
    narrow_packed = packed.desc.nbytes + packed.bits.nbytes
    rest = packed.n_bytes - narrow_packed
    med = {k: float(np.median(v)) for k, v in wall.items()}
    return {
        "workload": label, "records": packed.n_rec, "blocks": int(packed.blk_base[5]),
        "narrow_bytes_plain": int(narrow_plain), "narrow_bytes_packed": int(narrow_packed), "other_bytes": int(rest),
        "encoded_bytes": int(ds["len"].sum()),
        "a_host_unpack_then_append_plain_ms": spread(wall["a"]), "a_host_unpack_part_ms": spread(wall["a_unpack"]),
        "a_kernel_ms": {k: spread(v) for k, v in kern["a"].items() if any(v)},
        "b_append_packed_ms": spread(wall["b"]), "b_kernel_ms": {k: spread(v) for k, v in kern["b"].items() if any(v)},
        "c_unpack_device_wall_ms": spread(wall["c"]), "c_unpack_device_kernel_ms": spread(kern["c"]),
        "a_over_b": round(med["a"] / med["b"], 3), "a_minus_b_ms": round(med["a"] - med["b"], 3),
    }


def trace(eng, src):
    """(c) beside the plain columns written to device memory by the decode, a few times each."""
    n = len(src)
    packed = eng.decode_logs_columns(src, [1] * n, packed=True, payloads=True)
    p_dev, c_dev, keep = device_unpack_args(packed)
    h, ep = np.array([lg.handle for lg in src], np.uint32), np.ones(n, np.int64)
    sb = np.zeros((n + 1) * 5, np.uint64)
    c = _lib.Columns()
    for (name, _), o, cnt, cap in zip(PACK_STREAM_FIELDS, keep[2], packed.n_val, CAPS):
        setattr(c, name, o.data_ptr())
        setattr(c, cap, max(cnt, 1))
    wide = [torch.empty(8 * max(len(packed.w_v0), 1), dtype=torch.uint8, device="cuda") for _ in range(7)]
    for name, o in zip(("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0"), wide):
        setattr(c, name, o.data_ptr())
    c.cap_wide, c.span_base, c.out_kind = max(len(packed.w_v0), 1), sb.ctypes.data, _lib.CLG_MEM_DEVICE
    bad = _lib.UnpackBad()
    for _ in range(WARM + REPS):
        _lib.check(_lib.lib.clg_decode_logs_columns(eng.handle, h.ctypes.data, ep.ctypes.data, n, C.byref(c)))
        _lib.check(eng.unpack_columns_raw(p_dev, c_dev, bad))
    eng.sync()


def open_logs(eng, bufs, first, fill=True):
    logs = []
    for v, b in enumerate(bufs):
        lg = eng.open_log(CausalLogID.main(first + v))
        if fill:
            lg.processUpstreamDelta(b.tobytes(), 0, 1)
        logs.append(lg)
    return logs


res = {"reps": REPS, "warmup_rounds": WARM,
       "note": ("wall: host clock around synchronous calls, (a), (b) and (c) alternating in one process; the packed and the "
                "plain columns are host arrays; every round appends into a fresh epoch of the destination logs; kernel ms: "
                "HIP-event time of all kernels of a call under each stat; the host unpack runs on one thread of the GPU "
                "machine's host.")}
rng = np.random.default_rng(synth.SEED_CONFIG2)
bufs = [synth.config2_log(n_rec, rng)[0] for _ in range(n_logs)]
seg = 16384
c3 = None if TRACE else synth.config3_epoch(c3_rec, np.random.default_rng(3))[0]
rounds = 1 if TRACE else 2 * (WARM + REPS) + 1
pool = rounds * (sum(int(b.size) // seg + 2 for b in bufs) + (0 if c3 is None else c3_logs * (int(c3.size) // seg + 2))) + 64
with Engine(segment_bytes=seg, pool_segments=pool, timing=True) as eng:
    src = open_logs(eng, bufs, 0)
    if TRACE:
        trace(eng, src)
        sys.exit(0)
    res["config2"] = measure(eng, src, open_logs(eng, bufs, 2000, False), open_logs(eng, bufs, 4000, False),
                             f"config 2: {n_logs} logs x {n_rec} records, {sum(int(b.size) for b in bufs)} bytes")
    src3 = open_logs(eng, [c3] * c3_logs, 1000)
    res["config3"] = measure(eng, src3, open_logs(eng, [c3] * c3_logs, 3000, False), open_logs(eng, [c3] * c3_logs, 5000, False),
                             f"config 3: {c3_logs} logs, each one epoch of {c3_rec} records ({int(c3.size)} bytes), "
                             "with the payload column")

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "unpack_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
