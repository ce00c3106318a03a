"""Developer probe: the payload column (clg_decode_logs_columns_var) against what a columns caller
pays for the wide rows' payload bytes today, on two workloads:

  config3       config 3's logs (synth.config3_epoch: timers, checkpoints and Serializable streams)
  config2_timer a config-2-like batch (Order / Timestamp) with one named TimerTrigger per 1 000 records

in one process and alternating, 10 repeats after 3 warm-up rounds, each figure as median (min - max):

  (a) columns_to_host       clg_decode_logs_columns into registered host memory: today's call, no payloads
  (b) columns_var_to_host   clg_decode_logs_columns_var into registered host memory
  (c) columns_plus_logs     (a) plus clg_get_determinants_batch of the whole logs into registered host
                            memory: what keep_bytes=True costs, the baseline to compare (b) with
  (d) payload_kernels       the decode_payloads kernels alone (HIP events; clg_gather_payloads_logs over
                            device rows into device memory), beside a clg_get_determinants_batch into
                            device memory of about the same number of bytes (slice_gather)

(a)-(c): the host clock around calls that end in a synchronise.  Writes profiles/payload_probe.json and
prints it."""
import ctypes as C
import json
import mmap
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, synth  # noqa: E402

REPS, WARM = 10, 3
N_LOGS = int(os.environ.get("PROBE_LOGS", 32))
N_REC = int(os.environ.get("PROBE_REC", 250_000))
SEG = 16384


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def config2_timer_log(n, rng):
    """Order / Timestamp as config 2, every 1 000th record a TimerTrigger named "PTS"."""
    kinds = [synth.KINDS["order"], synth.KINDS["timestamp"], synth.KINDS["timer_pts"]]
    idx = (rng.random(n) < 0.5).astype(np.int64)
    idx[999::1000] = 2
    n_o, n_t = int((idx == 0).sum()), int((idx == 1).sum())
    return synth.build(idx, kinds, {0: [rng.integers(0, 4, n_o)],
                                    1: [1_700_000_000_000 + np.cumsum(rng.integers(0, 6, n_t))]})[0]


def registered(nbytes):
    buf = np.frombuffer(mmap.mmap(-1, (nbytes + 8191) & ~4095), np.uint8)
    buf[:] = 0  # fault the pages in before they are pinned
    _lib.check(_lib.lib.clg_host_register(buf.ctypes.data, buf.size))
    return buf


def carve(base, sizes):
    at, out = 0, []
    for s in sizes:
        out.append(base + at)
        at = (at + s + 255) & ~255
    return out, at


COLS = (("tag", 1, None), ("order", 1, 0), ("timestamp", 8, 1), ("rng", 4, 2), ("buffer_built", 4, 3), ("w_idx", 4, 4),
        ("w_rc", 4, 4), ("w_v1", 8, 4), ("w_var_off", 4, 4), ("w_var_len", 4, 4), ("w_sub", 1, 4), ("w_v0", 8, 4))


def run(name, bufs):
    n_logs = len(bufs)
    total = sum(int(b.size) for b in bufs)
    pool = sum(int(b.size) // SEG + 2 for b in bufs) + 64
    with Engine(segment_bytes=SEG, pool_segments=pool, timing=True) as eng:
        logs = []
        for v, b in enumerate(bufs):
            lg = eng.open_log(CausalLogID.main(v))
            lg.processUpstreamDelta(b.tobytes(), 0, 1)
            logs.append(lg)
        h = np.array([lg.handle for lg in logs], np.uint32)
        ep = np.ones(n_logs, np.int64)

        # sizes of the columns and the payloads, from one sizes-only call
        sz, psz = _lib.Columns(), _lib.Payloads()
        sb = np.zeros((n_logs + 1) * 5, np.uint64)
        sz.span_base = sb.ctypes.data
        _lib.check(_lib.lib.clg_decode_logs_columns_var(eng.handle, h.ctypes.data, ep.ctypes.data, n_logs, C.byref(sz),
                                                        C.byref(psz)))
        n, n_class = int(sz.n_rec), [int(x) for x in sz.n_class]
        n_rows, n_var = int(psz.n_rows), int(psz.n_var)
        assert n_rows == n_class[4]

        counts = [n if cls is None else n_class[cls] for _, _, cls in COLS]
        col_sizes = [max(c, 1) * w for c, (_, w, _) in zip(counts, COLS)]
        hcol = registered(carve(0, col_sizes)[1])
        cp, _ = carve(hcol.ctypes.data, col_sizes)
        cols = _lib.Columns()
        for (fname, _, _), p in zip(COLS, cp):
            setattr(cols, fname, p)
        cols.cap_tag, cols.cap_order, cols.cap_timestamp, cols.cap_rng, cols.cap_buffer_built = n, *n_class[:4]
        cols.cap_wide, cols.span_base, cols.out_kind = n_class[4], sb.ctypes.data, _lib.CLG_MEM_MAPPED
        hpay = registered(carve(0, [n_var + 1, 8 * (n_rows + 1)])[1])
        (pv, pp), _ = carve(hpay.ctypes.data, [n_var + 1, 8 * (n_rows + 1)])
        pay = _lib.Payloads()
        pay.var, pay.pos, pay.cap_var, pay.cap_pos, pay.out_kind = pv, pp, n_var, n_rows + 1, _lib.CLG_MEM_MAPPED
        hlog = registered(total + 1)
        ln, tot = np.zeros(n_logs, np.uint32), C.c_uint64()

        # (d): device rows (the decode's side table), device outputs
        o = [torch.empty(max(n, 1), dtype=t, device="cuda") for t in (torch.int32, torch.uint8, torch.int64)]
        w = [torch.empty(max(n_rows, 1), dtype=t, device="cuda") for t in
             (torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.uint8)]
        d = _lib.Decoded()
        d.off, d.tag, d.v0 = [x.data_ptr() for x in o]
        d.w_idx, d.w_rc, d.w_v1, d.w_var_off, d.w_var_len, d.w_sub = [x.data_ptr() for x in w]
        d.cap, d.wcap, d.out_kind = n, max(n_rows, 1), _lib.CLG_MEM_DEVICE
        eng.decode_logs_device(h, ep, d, np.zeros(n_logs + 1, np.uint64))
        row_base = np.ascontiguousarray(sb.reshape(-1, 5)[:, 4])
        dvar = torch.empty(max(n_var, 1), dtype=torch.uint8, device="cuda")
        dpos = torch.empty(n_rows + 1, dtype=torch.int64, device="cuda")
        dpay = _lib.Payloads()
        dpay.var, dpay.pos, dpay.cap_var, dpay.cap_pos = dvar.data_ptr(), dpos.data_ptr(), n_var, n_rows + 1
        dpay.out_kind = _lib.CLG_MEM_DEVICE
        # logs whose bytes add up to about n_var, for the gather beside the payload kernels
        k_logs = int(np.searchsorted(np.cumsum([b.size for b in bufs]), n_var)) + 1
        k_logs = min(k_logs, n_logs)
        dlog = torch.empty(sum(int(b.size) for b in bufs[:k_logs]) + 1, dtype=torch.uint8, device="cuda")

        def get_logs(out_ptr, cap, kind, k):
            _lib.check(_lib.lib.clg_get_determinants_batch(eng.handle, h.ctypes.data, ep.ctypes.data, k, out_ptr, cap, kind,
                                                           None, ln.ctypes.data, C.byref(tot)))
            return int(tot.value)

        def stat_ms(key):
            st = eng.kernel_stats()
            return st[key]["ms"] if key in st else float("nan")

        ms = {k: [] for k in ("a", "b", "c", "d_payload_kernels", "d_gather_kernels")}
        gathered = 0
        for r in range(WARM + REPS):
            if r == WARM:
                ms = {k: [] for k in ms}
            eng.sync()
            t0 = time.perf_counter()
            assert eng.decode_logs_columns_raw(h, ep, cols) == 0                                   # (a)
            t1 = time.perf_counter()
            _lib.check(_lib.lib.clg_decode_logs_columns_var(eng.handle, h.ctypes.data, ep.ctypes.data, n_logs,
                                                            C.byref(cols), C.byref(pay)))           # (b)
            t2 = time.perf_counter()
            assert eng.decode_logs_columns_raw(h, ep, cols) == 0                                   # (c)
            assert get_logs(hlog.ctypes.data, total, _lib.CLG_MEM_MAPPED, n_logs) == total
            t3 = time.perf_counter()
            ms["a"].append((t1 - t0) * 1e3)
            ms["b"].append((t2 - t1) * 1e3)
            ms["c"].append((t3 - t2) * 1e3)
            eng.kernel_stats_reset()                                                               # (d)
            assert eng.gather_payloads_logs(h, ep, d.w_var_off, d.w_var_len, row_base, device=True, out=dpay) == 0
            ms["d_payload_kernels"].append(stat_ms("decode_payloads"))
            eng.kernel_stats_reset()
            gathered = get_logs(dlog.data_ptr(), dlog.numel(), _lib.CLG_MEM_DEVICE, k_logs)
            eng.sync()
            ms["d_gather_kernels"].append(stat_ms("slice_gather"))

        # the payloads delivered are the logs' bytes at the columns' offsets
        var = np.frombuffer(C.string_at(pv, n_var), np.uint8)
        pos = np.frombuffer(C.string_at(pp, 8 * (n_rows + 1)), np.uint64)
        wo = np.frombuffer(C.string_at(cp[8], 4 * n_rows), np.uint32)
        wl = np.frombuffer(C.string_at(cp[9], 4 * n_rows), np.uint32)
        assert int(pos[-1]) == n_var == int(wl.sum())
        for s in (0, n_logs - 1):
            a, b = int(row_base[s]), int(row_base[s + 1])
            for k in list(range(a, min(a + 50, b))) + list(range(max(b - 50, a), b)):
                assert (var[int(pos[k]):int(pos[k + 1])] == bufs[s][int(wo[k]):int(wo[k]) + int(wl[k])]).all()
        assert (dvar.cpu().numpy()[:n_var] == var).all()

        col_bytes = sum(c * wd for c, (_, wd, _) in zip(counts, COLS))
        pay_bytes = n_var + 8 * (n_rows + 1)
        out = {
            "workload": f"{name}: {n_logs} logs, {n} records, {total} bytes in {SEG}-byte segments",
            "records": n, "wide_rows": n_rows, "payload_bytes": n_var, "log_bytes": total,
            "payload_share_of_log_bytes": round(n_var / total, 4),
            "a_columns_to_host_ms": spread(ms["a"]), "a_bytes_delivered": col_bytes,
            "b_columns_var_to_host_ms": spread(ms["b"]), "b_bytes_delivered": col_bytes + pay_bytes,
            "c_columns_plus_logs_ms": spread(ms["c"]), "c_bytes_delivered": col_bytes + total,
            "b_over_c_bytes": round((col_bytes + pay_bytes) / (col_bytes + total), 4),
            "c_over_b_wall": round(float(np.median(ms["c"]) / np.median(ms["b"])), 3),
            "b_over_a_wall": round(float(np.median(ms["b"]) / np.median(ms["a"])), 3),
            "d_payload_kernels_ms": spread(ms["d_payload_kernels"]), "d_payload_bytes_written": pay_bytes,
            "d_gather_kernels_ms": spread(ms["d_gather_kernels"]), "d_gather_bytes": gathered,
        }
        for b in (hcol, hpay, hlog):
            _lib.lib.clg_host_unregister(b.ctypes.data)
        return out


rng = np.random.default_rng(synth.SEED_CONFIG2)
res = {"reps": REPS, "warmup_rounds": WARM,
       "note": ("(a)-(c): host clock around synchronous calls into host memory registered with clg_host_register; "
                "(d): HIP-event time of all kernels of a call under one stat.")}
res["config3"] = run("config 3", [synth.config3_epoch(N_REC, rng)[0] for _ in range(N_LOGS)])
res["config2_timer"] = run("config 2 with a named TimerTrigger per 1000 records",
                           [config2_timer_log(4 * N_REC, rng) for _ in range(N_LOGS)])

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "payload_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
