"""Developer probe: the encode of typed columns (clg_encode_columns, clg_append_columns) against the
encode of SoA rows (clg_encode_batch), on two workloads:

  config2   config 2's logs (synth.config2_log: Order / Timestamp), PROBE_LOGS x PROBE_REC records
  config3   config 3's logs (synth.config3_epoch: timers, checkpoints and Serializable streams), the
            workload of tools/payload_probe.py

in one process and alternating, 10 repeats after 3 warm-up rounds, each figure as median (min - max):

  (a) soa_host_to_host      the former Engine.encode_columns: DecodedColumns.to_soa() in numpy, then
                            clg_encode_batch from host rows to host bytes (host clock); beside it
                            Engine.encode_columns as it is now (host columns to host bytes)
  (b) encode_batch_device   clg_encode_batch, device SoA to device bytes: the host clock around the call
                            (it has one host sync between sizes and write) and its encode_write kernel
  (c) encode_columns_device clg_encode_columns, device columns to device bytes: the same host clock, and
                            the encode_columns kernels (sizes and write sections, HIP events)
  (d) append                host columns into logs with clg_append_columns against clg_encode_batch +
                            clg_append_batch + flush for the same records (host clock), with the bytes
                            that cross the link for each

(a) and (d) run on the first PROBE_HOST_LOGS logs (host work per record dominates them).  The bytes
of (b) and (c) are compared on the device, and with the logs' own.  Writes
profiles/encode_columns_probe.json and prints it."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, synth  # noqa: E402
from clonos_amd.engine import DecodedColumns, _columns_in  # noqa: E402

REPS, WARM = 10, 3
N_LOGS = int(os.environ.get("PROBE_LOGS", 64))
N_REC = int(os.environ.get("PROBE_REC", 1_000_000))
HOST_LOGS = int(os.environ.get("PROBE_HOST_LOGS", 8))
SEG = 16384


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda") if a.size else \
        torch.empty(1, dtype=torch.uint8, device="cuda")


def sub_columns(cols, k):
    """The first k spans of cols as columns of their own."""
    b = cols.span_base[k].astype(np.int64)
    c = DecodedColumns(cols.tag[:int(b.sum())], cols.order[:b[0]], cols.timestamp[:b[1]], cols.rng[:b[2]],
                       cols.buffer_built[:b[3]], *[getattr(cols, f)[:b[4]] for f in
                                                   ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")],
                       cols.span_base[:k + 1])
    c.var_pos = cols.var_pos[:b[4] + 1]
    c.var = cols.var[:int(c.var_pos[-1])]
    return c


def old_encode_columns(eng, cols):
    b = cols.to_soa()
    return eng.encode_batch(b.tag, b.v0, b.w_idx, b.w_rc, b.w_v1, cols.var_pos[:-1].astype(np.uint32), b.w_var_len, b.w_sub,
                            cols.var.tobytes())


def run(name, bufs):
    n_logs = len(bufs)
    total = sum(int(b.size) for b in bufs)
    hk = min(HOST_LOGS, n_logs)
    host_total = sum(int(b.size) for b in bufs[:hk])
    rounds = WARM + REPS
    pool = sum(int(b.size) // SEG + 2 for b in bufs) + 2 * rounds * (host_total // SEG + 2 * hk) + 64
    with Engine(segment_bytes=SEG, pool_segments=pool, timing=True) as eng:
        logs = []
        for v, b in enumerate(bufs):
            lg = eng.open_log(CausalLogID.main(v))
            lg.processUpstreamDelta(b.tobytes(), 0, 1)
            logs.append(lg)
        cols = eng.decode_logs_columns(logs, [1] * n_logs, payloads=True)
        n, nw, n_var = cols.n_rec, len(cols.w_v0), len(cols.var)
        soa = cols.to_soa()

        # device SoA (clg_encode_in) and device columns (clg_columns_in)
        keep = [dev(x) for x in (soa.tag, soa.v0, soa.w_idx, soa.w_rc, soa.w_v1, cols.var_pos[:-1].astype(np.uint32),
                                 soa.w_var_len, soa.w_sub, cols.var)]
        p = [t.data_ptr() for t in keep]
        ein = _lib.EncodeIn(p[0], p[1], n, p[2], p[3], p[4], p[5], p[6], p[7], nw, p[8], n_var, _lib.CLG_MEM_DEVICE, 0)
        cin, hold = _columns_in(cols)
        ckeep = {}
        for f in ("tag", "order", "timestamp", "rng", "buffer_built", "w_rc", "w_v1", "w_var_len", "w_sub", "w_v0", "w_idx",
                  "pos", "var"):
            src = {"pos": cols.var_pos, "var": cols.var}.get(f)
            ckeep[f] = dev(np.asarray(getattr(cols, f) if src is None else src))
            setattr(cin, f, ckeep[f].data_ptr())
        cin.in_kind = _lib.CLG_MEM_DEVICE
        out_b = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
        out_c = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sbb = np.zeros(n_logs + 1, np.uint64)
        enc = _lib.Encoded()
        enc.bytes, enc.cap, enc.out_kind, enc.span_byte_base = out_c.data_ptr(), total, _lib.CLG_MEM_DEVICE, sbb.ctypes.data
        n_out, bad = C.c_uint64(), C.c_uint64()

        hcols = sub_columns(cols, hk)
        hsoa = hcols.to_soa()
        hlogs = [eng.open_log(CausalLogID.main(1000 + v)) for v in range(hk)]
        hlogs2 = [eng.open_log(CausalLogID.main(2000 + v)) for v in range(hk)]
        hbase = hcols.span_rec_base.astype(np.int64)

        def stat(key):
            st = eng.kernel_stats()
            return st[key]["ms"] if key in st else float("nan")

        names = ("a_soa_host_to_host", "a_columns_host_to_host", "b_wall", "b_encode_write_kernel", "c_wall", "c_kernels",
                 "d_append_columns", "d_encode_batch_append_flush")
        ms = {k: [] for k in names}
        for r in range(rounds):
            if r == WARM:
                ms = {k: [] for k in ms}
            eng.sync()
            t0 = time.perf_counter()
            a_old = old_encode_columns(eng, hcols)                                                       # (a)
            t1 = time.perf_counter()
            a_new = eng.encode_columns(hcols)
            t2 = time.perf_counter()
            assert a_old == a_new and len(a_new) == host_total
            ms["a_soa_host_to_host"].append((t1 - t0) * 1e3)
            ms["a_columns_host_to_host"].append((t2 - t1) * 1e3)
            eng.kernel_stats_reset()
            t0 = time.perf_counter()
            _lib.check(_lib.lib.clg_encode_batch(eng.handle, C.byref(ein), out_b.data_ptr(), total, _lib.CLG_MEM_DEVICE,
                                                 C.byref(n_out), C.byref(bad)))                          # (b)
            t1 = time.perf_counter()
            ms["b_wall"].append((t1 - t0) * 1e3)
            ms["b_encode_write_kernel"].append(stat("encode_write"))
            eng.kernel_stats_reset()
            t0 = time.perf_counter()
            assert eng.encode_columns_raw(cin, enc) == 0                                                 # (c)
            t1 = time.perf_counter()
            ms["c_wall"].append((t1 - t0) * 1e3)
            ms["c_kernels"].append(stat("encode_columns"))
            ep = np.full(hk, 10 + r, np.int64)
            t0 = time.perf_counter()
            nb = eng.append_columns(hlogs, ep, hcols)                                                    # (d)
            t1 = time.perf_counter()
            data = np.frombuffer(eng.encode_batch(hsoa.tag, hsoa.v0, hsoa.w_idx, hsoa.w_rc, hsoa.w_v1,
                                                  hcols.var_pos[:-1].astype(np.uint32), hsoa.w_var_len, hsoa.w_sub,
                                                  hcols.var.tobytes()), np.uint8)
            offs = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.uint64)
            eng.append_batch(np.array([lg.handle for lg in hlogs2], np.uint32), ep, offs, nb.astype(np.uint32), data)
            eng.sync()
            t2 = time.perf_counter()
            ms["d_append_columns"].append((t1 - t0) * 1e3)
            ms["d_encode_batch_append_flush"].append((t2 - t1) * 1e3)

        assert n_out.value == total == int(enc.n_bytes)
        torch.cuda.synchronize()
        assert torch.equal(out_b[:total], out_c[:total])
        assert out_c[:bufs[0].size].cpu().numpy().tobytes() == bufs[0].tobytes()
        assert (sbb == np.concatenate([[0], np.cumsum([b.size for b in bufs])])).all()
        for a, b in zip(hlogs, hlogs2):
            assert a.getDeterminants(10 + rounds - 1) == b.getDeterminants(10 + rounds - 1) == bufs[hlogs.index(a)].tobytes()
        hn, hw, hv = hcols.n_rec, len(hcols.w_v0), len(hcols.var)
        col_bytes = lambda c: sum(np.asarray(getattr(c, f)).nbytes for f in  # noqa: E731
                                  ("tag", "order", "timestamp", "rng", "buffer_built", "w_rc", "w_v1", "w_var_len", "w_sub",
                                   "w_v0", "w_idx")) + c.var_pos.nbytes + c.var.nbytes
        soa_bytes = 9 * hn + 25 * hw + hv
        out = {"workload": f"{name}: {n_logs} logs, {n} records, {total} bytes; host lines on {hk} logs, {hn} records",
               "records": n, "wide_rows": nw, "payload_bytes": n_var, "encoded_bytes": total,
               "columns_bytes_per_record": round(col_bytes(cols) / n, 3),
               "soa_bytes_per_record": round((9 * n + 25 * nw + n_var) / n, 3)}
        for k in names:
            out[k + "_ms"] = spread(ms[k])
        out["c_over_b_wall"] = round(float(np.median(ms["c_wall"]) / np.median(ms["b_wall"])), 3)
        out["d_link_bytes_append_columns"] = col_bytes(hcols)
        out["d_link_bytes_encode_batch_append_flush"] = soa_bytes + 2 * host_total  # rows up, bytes down, bytes up
        out["d_old_over_new_wall"] = round(float(np.median(ms["d_encode_batch_append_flush"]) /
                                                 np.median(ms["d_append_columns"])), 3)
        return out


rng = np.random.default_rng(synth.SEED_CONFIG2)
res = {"reps": REPS, "warmup_rounds": WARM,
       "note": ("wall: host clock around synchronous calls; kernel: HIP-event time of the kernels a call ran under one "
                "stat (clg_encode_batch times its write pass only, clg_encode_columns its sizes and write sections).")}
res["config2"] = run("config 2", [synth.config2_log(N_REC, rng)[0] for _ in range(N_LOGS)])
res["config3"] = run("config 3", [synth.config3_epoch(N_REC // 4, rng)[0] for _ in range(N_LOGS // 2)])

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "encode_columns_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
