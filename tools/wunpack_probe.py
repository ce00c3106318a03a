"""Developer probe: packed wide rows as input, in one process and alternating, REPS
repeats after WARM warm-up rounds, each figure as median (min - max).  On config 3 (PROBE_C3_LOGS
logs of one PROBE_C3_REC-record epoch, with the payload column) and on config 2 (PROBE_LOGS logs x
PROBE_REC records, no wide rows: the control), over what decode_logs_columns(packed=True,
pack_wide=True, payloads=True) delivered:

  end to end, into fresh destination logs whose digests are held against the sources':
  (a) host      Engine.append_columns(got): the wide rows through clg_unpack_wide_host and a rebuilt
                var_pos, then clg_append_columns_packed
  (b) device    Engine.append_columns(got, wide="device"): clg_append_columns_packed_wide

  kernels, device in and device out, on config 3's rows:
  clg_unpack_wide with and without pos beside its yardstick clg_pack_wide, which moves the same
  bytes the other way; algorithmic bytes over kernel time as a share of 8 TB/s.

Writes profiles/wunpack_probe.json and prints it."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = int(os.environ.get("PROBE_REPS", 10)), int(os.environ.get("PROBE_WARM", 3))
n_logs, n_rec = int(os.environ.get("PROBE_LOGS", 16)), int(os.environ.get("PROBE_REC", 250_000))
c3_logs, c3_rec = int(os.environ.get("PROBE_C3_LOGS", 16)), int(os.environ.get("PROBE_C3_REC", 250_000))
HBM_BYTES_PER_S = 8e12

import torch  # noqa: E402  (the engine binds torch's HIP runtime; device arrays for the kernel figures)
from clonos_amd import CausalLogID, Engine, _lib, synth  # noqa: E402

WIDE = (("w_idx", np.uint32), ("w_rc", np.int32), ("w_v1", np.int64), ("w_var_off", np.uint32),
        ("w_var_len", np.uint32), ("w_sub", np.uint8), ("w_v0", np.int64))
ROW_BYTES = sum(np.dtype(dt).itemsize for _, dt in WIDE)  # 33


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def open_sources(eng, bufs, first):
    logs = []
    for v, b in enumerate(bufs):
        lg = eng.open_log(CausalLogID.main(first + v))
        lg.processUpstreamDelta(b.tobytes(), 0, 1)
        logs.append(lg)
    return logs


def forget_host_rows(got):
    """What the host route builds and keeps on the columns: each repeat pays for it again."""
    for k in [name for name, _ in WIDE] + ["var_pos"]:
        got.__dict__.pop(k, None)


def end_to_end(eng, logs, label, next_vertex):
    n = len(logs)
    ep = [1] * n
    src = np.array([lg.handle for lg in logs], np.uint32)
    want = eng.digest_logs(src, np.ones(n, np.int64))
    got = eng.decode_logs_columns(logs, ep, packed=True, pack_wide=True, payloads=True)
    nw = got.wide_packed.n_wide
    ms = {"a_host": [], "b_device": [], "host_unpack": []}
    stats = {}
    for k in range(WARM + REPS):
        if k == WARM:
            ms = {x: [] for x in ms}
            stats = {}
        for variant in ("a_host", "b_device"):
            dst = [eng.open_log(CausalLogID.main(next_vertex[0] + i)) for i in range(n)]
            next_vertex[0] += n
            forget_host_rows(got)
            eng.sync()
            eng.kernel_stats_reset()
            t0 = time.perf_counter()
            if variant == "a_host":
                got.wide_packed.unpack() if nw else None  # (timed on its own: the share of (a) that is the host unpack)
                t1 = time.perf_counter()
                forget_host_rows(got)
                ms["host_unpack"].append((t1 - t0) * 1e3)
                t0 = time.perf_counter()
                eng.append_columns(dst, ep, got)
            else:
                eng.append_columns(dst, ep, got, wide="device")
            ms[variant].append((time.perf_counter() - t0) * 1e3)
            if variant == "b_device":
                assert "w_idx" not in got.__dict__ and "var_pos" not in got.__dict__
                for name, s in eng.kernel_stats().items():
                    if s["launches"]:
                        stats.setdefault(name, []).append(s["ms"])
            d = eng.digest_logs(np.array([lg.handle for lg in dst], np.uint32), np.ones(n, np.int64))
            assert (d["hash"] == want["hash"]).all() and (d["len"] == want["len"]).all(), variant
            for lg in dst:
                lg.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return got, {
        "workload": label, "records": got.n_rec, "wide_rows": nw, "payload_bytes": int(got.var.size),
        "delivered_bytes": got.n_bytes,
        "wall_ms": {k: spread(v) for k, v in ms.items()},
        "host_unpack_share_of_a": round(med["host_unpack"] / med["a_host"], 3),
        "wall_ratio_a_over_b": round(med["a_host"] / med["b_device"], 3),
        "b_kernel_ms_by_stat": {name: spread(v) for name, v in sorted(stats.items())},
    }


def kernels(eng, logs):
    """clg_unpack_wide and clg_pack_wide, device in and device out, on the same rows."""
    n = len(logs)
    plain = eng.decode_logs_columns(logs, [1] * n)
    nw, nr = len(plain.w_idx), plain.n_rec
    host = {name: np.ascontiguousarray(getattr(plain, name), dt) for name, dt in WIDE}
    host["tag"] = np.ascontiguousarray(plain.tag, np.uint8)
    dev = {name: torch.from_numpy(a.view(np.uint8)).cuda() for name, a in host.items()}  # (bytes: any element type)
    cin = _lib.Columns()
    for name, t in dev.items():
        setattr(cin, name, t.data_ptr())
    cin.n_rec, cin.out_kind = nr, _lib.CLG_MEM_DEVICE
    cin.n_class[4] = nw
    sizes = _lib.PackedWideC()
    _lib.check(eng.pack_wide_raw(cin, sizes))
    nb, nbits = int(sizes.blk_base[_lib.WPACK_STREAMS]), int(sizes.n_bits)
    d_desc = torch.empty(max(32 * nb, 16), dtype=torch.uint8, device="cuda")
    d_bits = torch.empty(max(nbits, 16), dtype=torch.uint8, device="cuda")
    pk = _lib.PackedWideC()
    pk.desc, pk.bits, pk.cap_desc, pk.cap_bits, pk.out_kind = d_desc.data_ptr(), d_bits.data_ptr(), nb, max(nbits, 16), _lib.CLG_MEM_DEVICE
    out = {name: torch.empty(max(nw, 1) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda") for name, dt in WIDE}
    pos = torch.empty(nw + 1, dtype=torch.int64, device="cuda")
    oc = _lib.Columns()
    for name, t in out.items():
        setattr(oc, name, t.data_ptr())
    oc.cap_wide, oc.out_kind = max(nw, 1), _lib.CLG_MEM_DEVICE
    bad = _lib.UnpackBad()
    ms = {"pack_wide": [], "unpack_wide": [], "unpack_wide_pos": []}
    for k in range(WARM + REPS):
        if k == WARM:
            ms = {x: [] for x in ms}
        for name in ms:
            eng.kernel_stats_reset()
            if name == "pack_wide":
                _lib.check(eng.pack_wide_raw(cin, pk))
            else:
                _lib.check(eng.unpack_wide_raw(pk, oc, pos.data_ptr() if name == "unpack_wide_pos" else None, bad))
            ms[name].append(eng.kernel_stats()[name.replace("_pos", "")]["ms"])
    for name, dt in WIDE:
        assert out[name].cpu().numpy()[:nw * np.dtype(dt).itemsize].tobytes() == host[name].tobytes(), name
    want_pos = np.concatenate([[0], np.cumsum(plain.w_var_len, dtype=np.uint64)]).astype(np.int64)
    assert (pos.cpu().numpy() == want_pos).all()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    alg = 32 * nb + nbits + ROW_BYTES * nw  # the packed form read, the plain rows written, once each
    return {
        "wide_rows": nw, "blocks": nb, "packed_bytes": 32 * nb + nbits, "plain_row_bytes": ROW_BYTES * nw,
        "kernel_ms": {k: spread(v) for k, v in ms.items()},
        "unpack_wide_over_pack_wide": round(med["unpack_wide"] / max(med["pack_wide"], 1e-9), 3),
        "unpack_wide_pos_over_pack_wide": round(med["unpack_wide_pos"] / max(med["pack_wide"], 1e-9), 3),
        "algorithmic_bytes": {"unpack_wide": alg, "unpack_wide_pos": alg + 8 * (nw + 1)},
        "share_of_8TBps": {"unpack_wide": round(alg / (med["unpack_wide"] * 1e-3) / HBM_BYTES_PER_S, 4),
                           "unpack_wide_pos": round((alg + 8 * (nw + 1)) / (med["unpack_wide_pos"] * 1e-3) / HBM_BYTES_PER_S, 4)},
    }


def control(eng, logs, got, next_vertex):
    """Config 2 has no wide rows: (b) against today's append_columns(packed), which it must equal."""
    n = len(logs)
    ep = [1] * n
    ms = {"append_columns_packed": [], "b_device": []}
    launches = 0
    for k in range(WARM + REPS):
        if k == WARM:
            ms = {x: [] for x in ms}
        for variant in ms:
            dst = [eng.open_log(CausalLogID.main(next_vertex[0] + i)) for i in range(n)]
            next_vertex[0] += n
            eng.sync()
            eng.kernel_stats_reset()
            t0 = time.perf_counter()
            eng.append_columns(dst, ep, got, wide="device" if variant == "b_device" else "host")
            ms[variant].append((time.perf_counter() - t0) * 1e3)
            launches += eng.kernel_stats().get("unpack_wide", {}).get("launches", 0)
            for lg in dst:
                lg.close()
    return {"wall_ms": {k: spread(v) for k, v in ms.items()}, "unpack_wide_launches": launches}


res = {"reps": REPS, "warmup_rounds": WARM,
       "note": ("wall: host clock around synchronous calls over host arrays, the variants alternating in one process, fresh "
                "destination logs each time, their digests held against the sources'; kernel ms: HIP-event time of all "
                "kernels of the call under each stat.")}
seg = 16384
c3 = synth.config3_epoch(c3_rec, np.random.default_rng(3))[0]
rng = np.random.default_rng(synth.SEED_CONFIG2)
bufs = [synth.config2_log(n_rec, rng)[0] for _ in range(n_logs)]
per_round = c3_logs * (int(c3.size) // seg + 2) + sum(int(b.size) // seg + 2 for b in bufs)
with Engine(segment_bytes=seg, pool_segments=32 * per_round + 1024, timing=True) as eng:
    vertex = [100_000]
    logs3 = open_sources(eng, [c3] * c3_logs, 1000)
    got3, res["config3"] = end_to_end(eng, logs3, f"config 3: {c3_logs} logs, each one epoch of {c3_rec} records "
                                      f"({int(c3.size)} bytes), with the payload column", vertex)
    res["config3"]["kernels_device_in_device_out"] = kernels(eng, logs3)
    logs2 = open_sources(eng, bufs, 0)
    got2, res["config2"] = end_to_end(eng, logs2, f"config 2: {n_logs} logs x {n_rec} records, no wide rows", vertex)
    res["config2"]["control"] = control(eng, logs2, got2, vertex)

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "wunpack_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
