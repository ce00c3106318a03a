// engine_impl.h -- what the engine's translation units (engine*.cpp) share: the error text,
// the device and pinned buffers, struct clg_engine with its data members, nested types and
// trivial accessors (every other method is defined in the unit that owns it), the call guards
// of the C ABI.  Included by those units only; everything it declares has hidden visibility.
#pragma once

#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <optional>
#include <vector>

#include "../../include/clonos_engine.h"
#include "engine_host.h"
#include "kernels.h"

using namespace clg_internal;  // the host-only types (engine_host.h)

#pragma GCC visibility push(hidden)

namespace clg_internal {

extern thread_local std::string g_err;  // the calling thread's error text (clg_last_error)
int fail(int code, const char* fmt, ...);

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return fail(CLG_E_DEVICE, "%s failed: %s", #x, hipGetErrorString(e_)); \
  } while (0)

void note_launch_error(const char* what);
#define CHK(x)                                          \
  do {                                                  \
    int r_ = (x);                                       \
    if (r_ != CLG_OK) {                                 \
      if (r_ == CLG_E_DEVICE) note_launch_error(#x);    \
      return r_;                                        \
    }                                                   \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return CLG_OK;
    if (p) hipFree(p);
    p = nullptr;
    size_t c = std::max(n, cap * 2);
    c = (c + 255) & ~size_t(255);
    hipError_t e = hipMalloc(&p, c + 64);
    if (e != hipSuccess) {
      cap = 0;
      return fail(CLG_E_DEVICE, "hipMalloc(%zu) failed: %s", c, hipGetErrorString(e));
    }
    cap = c;
    return CLG_OK;
  }
  ~DevBuf() {
    if (p) hipFree(p);
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  unsigned flags = hipHostMallocDefault;  // hipHostMallocCoherent: device atomics reach the host at once
  int ensure(size_t n) {
    if (n <= cap) return CLG_OK;
    if (p) hipHostFree(p);
    p = nullptr;
    size_t c = std::max(n, cap * 2);
    c = (c + 255) & ~size_t(255);
    hipError_t e = hipHostMalloc(&p, c, flags);
    if (e != hipSuccess) {
      cap = 0;
      return fail(CLG_E_DEVICE, "hipHostMalloc(%zu) failed: %s", c, hipGetErrorString(e));
    }
    cap = c;
    return CLG_OK;
  }
  ~PinBuf() {
    if (p) hipHostFree(p);
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

struct Stat {
  uint64_t launches = 0;
  double ms = 0;
  uint64_t bytes = 0;
};
struct PendingTiming {
  std::string name;
  hipEvent_t a, b;
  uint64_t bytes;
};


// The CLONOS_* developer switches, read from the environment once per engine: a member of
// clg_engine, filled when clg_engine_create constructs it.  No call reads the environment.
inline long long env_num(const char* name, long long dflt, int base = 10) {
  const char* v = getenv(name);
  return v ? strtoll(v, nullptr, base) : dflt;
}
inline std::string env_str(const char* name) {
  const char* v = getenv(name);
  return v ? v : "";
}
struct DevSwitches {
  bool robust_decode = env_str("CLONOS_DECODE") == "robust";  // the robust pipeline only
  bool small_decode = env_num("CLONOS_SMALL", 1) != 0;        // 0: no single-launch small batches
  bool sidecar = env_num("CLONOS_SIDECAR", 1) != 0;           // 0: no Serializable candidate lists (developer A/B)
  bool keep_errors = env_num("CLONOS_KEEP_ERRORS", 1) != 0;   // 0: decode errors not kept on the fast path
  bool columns_small = env_num("CLONOS_COLUMNS_SMALL", 1) != 0;  // 0: no one-launch columns / payloads for small batches
  bool pack_small = env_num("CLONOS_PACK_SMALL", 1) != 0;        // 0: no one-launch pack of small batches
  uint32_t fused_perturb = uint32_t(env_num("CLONOS_FUSED_PERTURB", 0, 0));  // test switch (FusedCtl::perturb)
  // initial spill arena bytes (tests: force its growth); 0: the default
  size_t jser_arena = getenv("CLONOS_JSER_ARENA") ? std::max<size_t>(256, size_t(env_num("CLONOS_JSER_ARENA", 0, 0))) : 0;
  int gather_prio = int(env_num("CLONOS_GATHER_PRIO", 1));     // the streams' priorities (clg_engine_create)
  // the batched slice's dispatch window in segments (slice_order.h; 0: request order, -1: the default)
  long long gather_window = env_num("CLONOS_GATHER_WINDOW", -1);
  int host_threads = int(env_num("CLONOS_HOST_THREADS", 16));  // host threads for the per-log loops
  int lean = int(env_num("CLONOS_LEAN", -1));  // 0/1: the count pass's lean walk forced off / on (-1: by the hint)
  int warm = int(env_num("CLONOS_WARM", -1));  // speculative warm-up bytes (-1: the default, spec_warm)
  bool host_prof = getenv("CLONOS_HOST_PROF") != nullptr;      // host-phase timing as "host_*" pseudo-stats
  bool fused_debug = getenv("CLONOS_FUSED_DEBUG") != nullptr;  // the fused decode's diagnostics block (ZDbg), printed
  bool small_prof = getenv("CLONOS_SMALL_PROF") != nullptr;    // the small path's phase stamps, printed
  // files for per-tile phase stamps and the robust scan's state (empty: off)
  std::string scan_phases = env_str("CLONOS_SCAN_PHASES"), robust_phases = env_str("CLONOS_ROBUST_PHASES"),
              debug_dump = env_str("CLONOS_DEBUG_DUMP");
};

}  // namespace clg_internal

// The device address of registered host memory [h, h + n) (0: not wholly inside one
// registered range).
uintptr_t clg_mapped_device_address(const void* h, uint64_t n);
// How many of the n bytes at h one copy may take: up to the first edge of a registered range
// inside them (the HIP runtime refuses a copy that crosses the end of registered memory).
uint64_t clg_mapped_piece(const void* h, uint64_t n);

struct clg_engine {
  clg_config cfg{};
  const DevSwitches sw;
  hipStream_t stream = nullptr;
  void* pool_alloc = nullptr;  // pool minus the guard bytes either side
  uint8_t* pool = nullptr;
  std::vector<uint32_t> free_segs;
  // The write path's Serializable candidates per segment (kernels.h SideCar; hdr null: none,
  // every decode tile is scanned), and each segment's life stamp: bumped whenever the segment
  // leaves the free list, carried by the chunks written into it.
  clg::SideCar side{};
  void* side_alloc = nullptr;
  std::vector<uint32_t> seg_life;
  const clg::SideCar* side_arg() const { return side.hdr ? &side : nullptr; }
  // a chunk's life word: the segment's life (31 bits) | 1 << 31 when the request's bytes go on
  // in the next chunk (contiguous in the source: the writer measures streams across it)
  uint32_t life_word(uint32_t seg, bool more) const { return (seg_life[seg] & 0x7FFFFFFFu) | (more ? 0x80000000u : 0u); }
  // the in-flight (data) log's own pool (clg_config.ifl_*)
  void* ifl_alloc = nullptr;
  uint8_t* ifl_pool = nullptr;
  uint32_t ifl_C = 0;
  std::vector<uint32_t> ifl_free;
  uint8_t* ifl_addr(uint32_t s) const { return ifl_pool + size_t(s) * ifl_C; }
  std::vector<Log> logs;
  std::vector<InFlight> ifls;
  std::map<IdKey, uint32_t> by_id;
  std::vector<Job> jobs;  // jobs[0]: the default job (cfg.sharing_depth)
  std::vector<uint32_t> dirty;  // logs with staged (unflushed) bytes: flush() visits only these
  EngineLock mu;
  std::mutex pool_mu;   // free_segs, taken by appends holding only their stripe
  std::mutex dirty_mu;  // dirty, idem

  // staging / scratch
  PinBuf h_stage, h_desc, h_sres, h_outs;
  // Per decode slot (0: synchronous calls; 1, 2: the asynchronous decodes in flight): the
  // read-back of span ranges and abort words, the staged plan, the end-of-read-back event.
  static constexpr uint32_t kSlots = 1 + CLG_DECODE_MAX_INFLIGHT;
  PinBuf h_zres_s[kSlots], h_plan_s[kSlots];
  hipEvent_t zdone[kSlots] = {};
  uint32_t plan_slot = 0;  // the slot stage_plan / enqueue_plan use (launch_fused sets it)
  DevBuf d_stage, d_desc, d_pieces, d_tiles, d_spans, d_agg, d_conv, d_tres, d_sres, d_totals, d_out;
  std::vector<uint64_t> tab_at;  // RunPlan: a log's place in the segment table (UINT64_MAX: none)
  DevBuf d_fconv, d_lanes, d_sums, d_fres, d_flags, d_dbg, d_prof, d_rprof, d_prof2, d_jpos, d_jlen, d_jn, d_defer;
  DevBuf d_o_off, d_o_tag, d_o_v0, d_o_widx, d_o_wrc, d_o_wv1, d_o_wvo, d_o_wvl, d_o_wsub;
  DevBuf d_zctl, d_ztiles, d_zbits;  // fast decode: control words, tiles, record-start bitmaps
  DevBuf d_zjpos, d_zjlen, d_zjn, d_zjwork;  // fast decode: Serializable length tables (phase 3)
  uint32_t zjovf_cap = 1u << 16;  // their overflow arena's entries (grown on demand)
  uint32_t zjwork_min = 0;        // the general walker's work list: at least this many items
  DevBuf d_zbad;                     // fast decode: per-span "chain went wrong" flags
  DevBuf d_sf_meta, d_sf_rec, d_sf_wide;  // per-span fallback: bad-span list, robust outputs
  bool jser_hint = false;            // the last batches held Serializable records: build tables first
  // The count pass's lean speculative walk (decode_fused.hip lean_walk) while the last fast
  // decode's records were almost all fixed-length (wide rows under 1/16): its result is the
  // same either way, its cost grows with wide records.  CLONOS_LEAN=0/1 forces it (developer).
  bool lean_hint = true;
  DevBuf d_rmeta, d_rsizes;          // replay-prep: subpartition span tables / BufferBuilt sizes
  DevBuf d_encin, d_encw, d_encout;  // encode: staged host input, block prefixes, host-output staging
  DevBuf d_hdr;                      // piggyback: delta headers staged for the gather
  // encode of typed columns: staged host input | span_base, per-tile counts / bases / sums, the
  // encoded bytes (host-output staging, and what clg_append_columns scatters); the scans' results
  // and the span bases (pinned: the kernels write them)
  DevBuf d_ecolin, d_ecolw, d_ecolout;
  PinBuf h_ecolres;
  // The Serializable walker's spill arena (kernels.h JArena): [used u64 | pad to 256 | bytes].
  // Grown (doubled) whenever a decode reports CLG_E_NOSPACE, i.e. a walk found it full.
  DevBuf d_jarena;
  size_t jarena_bytes = size_t(16) << 20;
  PinBuf h_jused;  // read-backs of the arena's bump counter: [0] decode, [1] replay classification
  // Slices into device memory run on their own stream, overlapping the next decode: the
  // gather only reads log segments, so every pool write (flush / upstream scatter) and
  // every full sync first waits for it (gwait).
  hipStream_t gstream = nullptr;
  hipEvent_t gready = nullptr;
  bool g_pending = false;
  // two descriptor sets, so a gather can be queued while the previous one still runs;
  // gdone[s] marks the end of the last gather that used set s
  PinBuf h_gdesc[2];
  DevBuf d_gdesc[2], d_gpieces[2];
  hipEvent_t gdone[2] = {nullptr, nullptr};
  uint32_t gseq = 0;
  PinBuf h_rmeta;
  PinBuf h_rout;  // replay-prep: the subpartition results, read back in one place (pinned)
  DevBuf d_plan;
  DevBuf d_dgtab, d_dgpart, d_dgout;  // log digest: the constant table (uploaded once), partials, results
  DevBuf d_dgsum;                     // prefix digests: a sum per stretch
  PinBuf h_dgout;
  bool dgtab_ready = false;
  DevBuf d_dffirst, d_dfout;  // log comparison: a word per piece, results
  PinBuf h_dfout;
  // typed columns: per-tile counts and bases, span boundaries and bases, the scan's results
  // (pinned: the kernel writes them), host-output staging
  DevBuf d_colcnt, d_colbase, d_colsrb, d_colsb, d_colout;
  PinBuf h_colres, h_colsb;
  // ... the one-launch form: result block | span bases | span boundaries (pinned: the kernel
  // reads and writes them), and the packed columns of a host caller read back in one copy
  PinBuf h_colsmall, h_colpack;
  // the payload column: span table | segment table | row_base (pinned, then device), the rows of
  // a host caller, per-tile sums / bad rows / bases, the scan's results, host-output staging
  DevBuf d_paydesc, d_payrows, d_paytile, d_payout;
  PinBuf h_paydesc, h_payres;
  PinBuf h_paypack;  // the one-launch form: pos | var of a host caller read back in one copy
  // packed columns: staged host input, the decode's narrow columns, the blocks' descriptors, the
  // scan groups' sums, host-output staging; the scan's total (pinned: the kernel writes it)
  DevBuf d_packin, d_packcol, d_packdesc, d_packsum, d_packout;
  PinBuf h_packres;
  // packed columns as input: staged host input, the plain narrow columns the packed encode reads,
  // host-output staging, and the check's verdict (device words, read back into pinned memory)
  DevBuf d_unpackin, d_unpackcol, d_unpackout, d_unpackres;
  PinBuf h_unpackres;
  // packed wide rows: staged host input, kind bytes | tile counts | tile bases | the bad-row word,
  // the per-kind field arrays, the stream table (pinned, then device), the blocks' descriptors,
  // the scan groups' sums, host-output staging; the scans' results (pinned: the kernels write them)
  DevBuf d_wpackin, d_wpackkind, d_wpacksoa, d_wpacktab, d_wpackdesc, d_wpacksum, d_wpackout;
  PinBuf h_wpacktab, h_wpackres;
  // both packs in one launch: the result block (pinned: the kernel writes it), and desc | bits of a
  // host caller read back in one copy a half
  PinBuf h_packsmall, h_packland;
  // packed wide rows as input: staged host input, kind bytes | tile counts | tile bases | tile
  // sums | the verdict words, the per-kind field arrays, the stream table (pinned, then device),
  // host-output staging, the rows and pos for the encode; the totals and the verdict (pinned)
  DevBuf d_wunpackin, d_wunpackwork, d_wunpacksoa, d_wunpacktab, d_wunpackout, d_wunpackrow;
  PinBuf h_wunpacktab, h_wunpackres;
  // the packed payload column: staged host input (var | pos, or desc | bits | tail), the unpack's
  // staged pos, lcps | descriptors | tile sums | tile bases | findings, host-output staging; the
  // scans' results (pinned: the kernels write them)
  DevBuf d_ppayin, d_ppaypos, d_ppaywork, d_ppayout;
  PinBuf h_ppayres;
  bool fused_decode = true;  // CLG_F_ROBUST_DECODE / CLONOS_DECODE=robust: robust pipeline only
  bool small_decode = true;  // CLG_F_NO_SMALL_DECODE / CLONOS_SMALL=0: no single-launch small batches

  // timing
  std::map<std::string, Stat> stats;
  // Developer host-phase timing (CLONOS_HOST_PROF set): the wall time of host-side work as
  // pseudo-stats "host_*" beside the kernels' (launches = calls, ms = host wall time).
  struct HostTimer {
    clg_engine* e;
    const char* name;
    std::chrono::steady_clock::time_point t0;
    HostTimer(clg_engine* en, const char* n) : e(en && en->sw.host_prof ? en : nullptr), name(n) {
      if (e) t0 = std::chrono::steady_clock::now();
    }
    ~HostTimer() {
      if (!e) return;
      Stat& s = e->stats[name];
      s.launches++;
      s.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // (sections of one call: the time since the last lap, under `lap_name`)
    void lap(const char* lap_name) {
      if (!e) return;
      const auto now = std::chrono::steady_clock::now();
      Stat& s = e->stats[lap_name];
      s.launches++;
      s.ms += std::chrono::duration<double, std::milli>(now - t0).count();
      t0 = now;
    }
  };
  std::vector<PendingTiming> timings;
  std::vector<hipEvent_t> ev_pool;

  uint32_t C() const { return cfg.segment_bytes; }
  uint8_t* seg_addr(uint32_t s) const { return pool + size_t(s) * C(); }
  // The scatter chunks that write n source bytes from offset src on at [at, at + n) of log l, whose
  // segments are attached: one per segment touched (for_each_chunk), written from ch on; returns the
  // place behind them.  Inline: a config-4 step builds 66 k requests' chunks.
  clg::ScatterChunk* add_chunks(clg::ScatterChunk* ch, const Log& l, uint32_t at, uint32_t n, uint64_t src) const {
    for_each_chunk(at, n, C(), [&](uint32_t si, uint32_t so, uint32_t take, bool more) {
      *ch++ = clg::ScatterChunk{seg_addr(l.segs[si]) + so, src, take, life_word(l.segs[si], more)};
      src += take;
    });
    return ch;
  }
  // The n chunks in h_desc uploaded to d_desc and their scatter of `total` bytes from d_src queued
  // under the stat `name` (side: with the write path's side car).  The caller waits as it needs to.
  int scatter_chunks(const char* name, size_t n, uint64_t total, const uint8_t* d_src, bool side);
  // The nine d_o_* decode scratch arrays grown to cap records and wcap wide rows, and their
  // addresses in o (o->cap, o->wcap are the caller's to set).
  int scratch_out(size_t cap, size_t wcap, clg::DecodeOut* o);
  hipEvent_t get_event();
  template <class F>
  int timed(const char* name, uint64_t bytes, F&& launch, hipStream_t on = nullptr) {
    if (!(cfg.flags & CLG_F_TIMING)) return launch();
    hipEvent_t a = get_event(), b = get_event();
    hipEventRecord(a, on ? on : stream);
    int r = launch();
    hipEventRecord(b, on ? on : stream);
    timings.push_back(PendingTiming{name, a, b, bytes});
    return r;
  }
  void collect_timings(bool ready_only = false);
  int gwait();
  int jarena_reset(clg::JArena* a);
  int jarena_note(int k);
  int jarena_clear_note(int k);
  bool jarena_spilled(int k) const { return h_jused.p && h_jused.as<uint64_t>()[k] > jarena_bytes; }
  int jarena_grow();
  int sync();

  // ---------------------------------------------------------------- segments
  int32_t capacity(const Log& l) const { return int32_t(l.segs.size()) * int32_t(C()); }
  int ensure_space(Log& l, int32_t n);
  int ensure_space_locked(Log& l, int32_t n);
  void write_pending(Log& l, const uint8_t* b, uint32_t n);
  // epochStartOffsets.computeIfAbsent(e -> visibleWriterIndex); valid until the next insert
  static EpochEnt* compute_if_absent(Log& l, int64_t e) { return l.epochs.emplace(e, l.writer); }
  int32_t bytes_to_send(const Log& l, int64_t epoch, int32_t phys) const {  // :384-395
    auto it = l.epochs.find(epoch + 1);
    return (it != l.epochs.end() ? it->offset : l.writer) - phys;
  }

  int get_log(uint32_t h, Log** out) {
    if (h >= logs.size() || !logs[h].open) return fail(CLG_E_NO_LOG, "unknown log handle %u", h);
    *out = &logs[h];
    return CLG_OK;
  }
  void trim_tail(Log& l);
  bool over_stage_limit(uint32_t h) const;
  // Forget the host tail (bytes were written to HBM behind its back).
  static void reset_tail(Log& l) {
    l.tail.clear();
    l.tail_start = l.writer;
  }
  int flush();
  int append(uint32_t h, int64_t epoch, const uint8_t* b, uint32_t n);
  int upstream(uint32_t h, int64_t epoch, int32_t off_from_epoch, const uint8_t* d, uint32_t n);
  int upstream_batch(clg_delta_req* r, uint32_t n, const uint8_t* bytes, uint32_t in_kind);

  // upstream_batch's device-input loop on the host threads, for batches of many distinct logs
  // (config 4: 66 k): per part each request's new bytes and the segments it needs; then, in
  // request order, the segments taken from the pool (a request the pool cannot serve gets
  // CLG_E_NOSPACE with nothing taken, a gap CLG_E_GAP after its segments were added -- as one by
  // one) and each request's place among the scatter chunks; then per part the segments
  // attached, the chunks written and the logs advanced.  false: not applicable (a log twice).
  std::vector<uint8_t> up_seen;
  struct UpPlan {
    int32_t num_new, writer, cur;  // (the log's writer and offset in the epoch, read in the first pass)
    uint32_t need, chunks;
    uint64_t seg_from, ch_from;
  };
  std::vector<UpPlan> up_plan;
  bool upstream_parallel(clg_delta_req* r, uint32_t n, const uint8_t* bytes, int* out_st);
  int has_delta(uint32_t h, ChKey k, int64_t epoch, int32_t* out);
  int offset_from_epoch(uint32_t h, ChKey k, int32_t* out);
  int take_delta(uint32_t h, ChKey k, int64_t epoch, int32_t* phys, int32_t* nb);
  void add_pieces(const Log& l, int32_t phys, int32_t n, uint64_t dst, std::vector<clg::GatherPiece>& out);

  // A gather's output: the launch writes to the caller's device buffer, or to d_out, which is
  // then copied to the caller's host buffer.  launch(dout) queues the kernel on `stream`;
  // wait = false returns without a sync when the output stays on the device.
  template <class L>
  int gather_out(void* out, uint32_t out_kind, uint64_t total, const char* stat, bool wait, L&& launch) {
    uint8_t* dout;
    if (out_kind == CLG_MEM_DEVICE) {
      dout = static_cast<uint8_t*>(out);
    } else {
      CHK(d_out.ensure(total));
      dout = d_out.as<uint8_t>();
    }
    CHK(timed(stat, 2 * total, [&] { return launch(dout); }));
    if (out_kind != CLG_MEM_DEVICE) HIPCHK(hipMemcpyAsync(out, dout, total, hipMemcpyDeviceToHost, stream));
    return wait || out_kind != CLG_MEM_DEVICE ? sync() : CLG_OK;
  }
  int run_gather(const std::vector<clg::GatherPiece>& pieces, uint64_t total, void* out, uint32_t out_kind,
                 const char* stat = "slice_gather", bool wait = true);

  // A gather's run plan: byte ranges of logs as runs for the device-side piece expansion
  // (k_expand_pieces), packed back to back in the output, with each log's segment indices once
  // in segtab: the log's place there is kept by handle in tab_at (a hash map took 0.1 ms for
  // config 5's 2 064 logs), whose touched entries are reset when the plan goes.
  struct RunPlan {
    clg_engine& e;
    std::vector<clg::SegSpan> runs;
    std::vector<uint32_t> segtab;
    uint32_t n_pieces = 0;
    uint64_t total = 0;  // bytes planned: the next run's place in the output
    std::vector<uint32_t> touched;
    RunPlan(clg_engine& en, uint32_t n) : e(en) {
      runs.reserve(n);
      touched.reserve(n);
      if (e.tab_at.size() < e.logs.size()) e.tab_at.resize(e.logs.size(), UINT64_MAX);
    }
    RunPlan(const RunPlan&) = delete;
    ~RunPlan() {
      for (uint32_t h : touched) e.tab_at[h] = UINT64_MAX;
    }
    // [phys, phys + nb) of log h for request `req` (the run's pad), at `total` in the output
    void add(uint32_t h, int32_t phys, int32_t nb, uint32_t req) {
      if (nb > 0) {
        uint64_t& at = e.tab_at[h];
        if (at == UINT64_MAX) {
          const SegList& segs = e.logs[h].segs;
          at = segtab.size();
          touched.push_back(h);
          segtab.insert(segtab.end(), segs.begin(), segs.end());
        }
        runs.push_back(clg::SegSpan{at, uint32_t(phys), uint32_t(nb), total, n_pieces, req});
        n_pieces += uint32_t(phys + nb - 1) / e.C() - uint32_t(phys) / e.C() + 1;
      }
      total += uint64_t(nb);
    }
  };

  struct DescSet {
    PinBuf& h;
    DevBuf &d, &pieces;
  };
  struct StagedPlan {
    const clg::SegSpan* runs;
    const clg::GatherPiece* pieces;
    const uint8_t* extra;
  };
  static size_t al16(size_t x) { return (x + 15) & ~size_t(15); }
  int stage_run_plan(const RunPlan& p, DescSet s, hipStream_t on, StagedPlan* sp, const void* extra = nullptr,
                     size_t extra_bytes = 0);
  int run_gather_runs(const RunPlan& p, void* out, uint32_t out_kind);
  int plan_determinant_runs(const uint32_t* log, const int64_t* start_epoch, uint32_t n, uint32_t* len,
                            uint64_t* out_off, RunPlan& p);
  int stage_spans(const uint8_t* bytes, const uint64_t* off, const uint64_t* len, uint32_t n, uint32_t in_kind,
                  const uint8_t** base, uint64_t* base_off);
  int ensure_dgtab();
  int digest_prefixes(const uint32_t* log, const int64_t* start_epoch, uint32_t n, const uint64_t* first,
                      const uint32_t* cuts, clg_digest* out);
  int run_digest(const clg::SegSpan* d_runs, uint32_t n_runs, const clg::GatherPiece* d_pc, uint32_t n_pieces,
                 uint64_t bytes, uint32_t n, clg_digest* out);
  int gather_runs_async(const RunPlan& p, void* out);

  // host_only: serve the slice from the host tail or return kNeedGpu with nothing changed
  // (the caller holds only the shared lock and retries under the exclusive one).
  static constexpr int kNeedGpu = 1;
  int get_delta(uint32_t h, ChKey k, int64_t epoch, void* out, uint32_t cap, uint32_t kind, uint32_t* n,
                bool host_only = false);
  int determinants_range(const Log& l, int64_t start_epoch, int32_t* start, int32_t* nb);
  int get_determinants(uint32_t h, int64_t start_epoch, void* out, uint32_t cap, uint32_t kind, uint32_t* n,
                       bool host_only = false);
  int checkpoint_complete(Log& l, int64_t cp);
  int checkpoint_complete(Log& l, int64_t cp, std::vector<uint32_t>& freed);

  // ---------------------------------------------------------------- decode
  struct DecodePlan {
    std::vector<clg::TileDesc> tiles;   // host-built tiles (staged host input)
    std::vector<clg::SpanDesc> spans;
    std::vector<clg::SegSpan> runs;     // log spans: tiles generated on the device
    std::vector<uint32_t> segtab;       // concatenated segment indices of the runs' logs
    uint32_t n_tiles = 0;
    uint32_t n_tiny = 0;                // whole spans of one tile and at most kZTinySpan bytes
    uint32_t unit = 0;                  // device-planning tile window
    const std::vector<uint32_t>* only = nullptr;  // plan only these spans (ascending), as spans 0, 1, ...
    // a builder that could not plan a log (a queued decode's re-plan after a rebase found its
    // range gone): the decode fails with this status instead of decoding an empty span
    int status = CLG_OK;
    // plan_parallel wrote the runs, segment table and spans straight into the pinned plan
    // buffer of decode slot stage_slot (stage_plan then adds only the chunk table); runs and
    // segtab stay empty, their sizes are n_runs / n_segs.  A re-launch of the plan (an abort's
    // fallbacks) re-plans it from its builder first (unstage).
    bool staged = false;
    uint32_t stage_slot = 0;
    size_t n_runs = 0, n_segs = 0;
    size_t run_count() const { return staged ? n_runs : runs.size(); }
    size_t seg_count() const { return staged ? n_segs : segtab.size(); }
    void reset() {  // empty, capacity kept (a config-4 plan is ~4 MB: fresh pages cost page faults)
      status = CLG_OK;
      staged = false;
      stage_slot = 0;
      n_runs = n_segs = 0;
      tiles.clear();
      spans.clear();
      runs.clear();
      segtab.clear();
      n_tiles = n_tiny = unit = 0;
      only = nullptr;
    }
  };
  // `build(plan, tile_bytes)` fills a plan for the given tile geometry (decode, decode_async)
  using PlanBuild = std::function<void(DecodePlan&, uint32_t)>;
  // clg_decode_logs' plan and log ranges, kept between calls for their capacity
  DecodePlan zplan;
  // host threads for batches of very many logs (CLONOS_HOST_THREADS, default 8; 1: none)
  std::unique_ptr<WorkPool> host_pool;
  static int usable_cpus();
  WorkPool* workers();
  static constexpr uint32_t kParallelLogs = 8192;  // logs per batch from which the loops split
  std::vector<int32_t> zst, znb;
  static bool plan_keep(const DecodePlan& p, uint32_t* s);
  uint32_t tile_unit(uint32_t k) const;
  void plan_host_span(DecodePlan& p, const uint8_t* dbase, uint64_t len, uint32_t s, uint32_t T);
  void plan_log_span(DecodePlan& p, const Log& l, int32_t start, int32_t len, uint32_t s, uint32_t T);
  bool plan_parallel(DecodePlan& p, const uint32_t* log, const int64_t* start_epoch, uint32_t n, uint64_t* total,
                     int stage = -1);
  static void reset_result(clg_decoded* out);
  int upload_plan(DecodePlan& p, DevBuf& dtiles);
  // Where a staged plan lies in h_plan / d_plan (byte offsets).
  struct PlanLayout {
    size_t tb = 0, sb = 0, o_runs = 0, o_seg = 0, o_spans = 0, o_chunk = 0, hb = 0;
  };
  static void plan_layout(size_t tb, size_t rb, size_t gb, size_t sb, size_t cb, PlanLayout* L);
  int stage_plan(const DecodePlan& p, DevBuf& dtiles, PlanLayout* L, const std::vector<uint32_t>* chunk = nullptr);
  static constexpr size_t kParallelCopy = 1u << 20;
  void count_chunks(const DecodePlan& p, uint32_t G, bool tiny, std::vector<uint32_t>& ch);
  std::vector<uint32_t> chunk_buf;
  int enqueue_plan(const DecodePlan& p, const PlanLayout& L, DevBuf& dtiles);

  // Output arrays the kernels write: the caller's device arrays, or engine scratch that
  // finish_out copies to the caller's host arrays.
  // Registered host outputs (CLG_MEM_MAPPED) of at most kMappedDirect bytes: the kernels write
  // them through their device addresses, so no read-back copy and no host memcpy follow (for
  // config 5's replay-prep decode, 1.7 MB of rows: 0.12 ms of finish_out).
  static constexpr uint64_t kMappedDirect = 8ull << 20;
  static bool mapped_direct(const clg_decoded& out);
  int prep_out(clg_decoded* out, clg::DecodeOut* o);

  // An asynchronous decode into device memory completes on its own stream only: slices still
  // running on gstream only read log segments, and every call that writes segments waits for
  // gstream first (flush, upstream deltas, the in-flight pool).  Measured on MI355X (config-2
  // step, 3 runs each, tools/ab_env.sh): 0.79 ms against 0.83 ms when the completion also
  // drained gstream.
  bool settling = false;  // settle() is completing an asynchronous decode
  int finish_out(clg_decoded* out, uint64_t nrec, uint64_t nwide);
  uint32_t spec_warm() const;
  int run_fused(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base, bool* aborted,
                bool jser, bool* need_jser);
  static void span_totals(const DecodePlan& p, const uint64_t* hz, uint64_t* span_rec_base, uint64_t* nrec,
                          uint64_t* nwide);
  static constexpr uint32_t kHostResSpans = 1024;  // spans up to which the scan writes the host read-back
  static bool fused_fits(const DecodePlan& p);

  // One queued three-pass decode: launch_fused queues everything up to the read-back of the
  // span ranges and abort words; finish_fused waits for it and turns it into the result.
  struct FusedRun {
    uint64_t log_bytes = 0;
    bool jser = false;
    hipEvent_t ea = nullptr, eb = nullptr;  // emit's timing events
    hipEvent_t pa = nullptr, pb = nullptr;  // the whole pipeline's (count start .. emit end)
    // for the per-span fallback: the run's control words and outputs, and whether only
    // span-local reasons aborted it (chains that went wrong, not a timeout / table overflow)
    clg::FusedCtl ctl{};
    clg::DecodeOut o{};
    bool span_local = false;
    bool lookback_bad = false;  // emit found a scan offset other than its predecessor's prefix
    // its decode slot (read-back buffer, staged plan, jser arena note), and for a queued
    // decode the event after its read-back, which its completion waits for (not the stream:
    // a later decode may be queued behind it)
    uint32_t slot = 0;
    hipEvent_t done = nullptr;
    int note() const { return slot ? int(1 + slot) : 0; }
  };
  FusedRun zlast;  // the last finished fast run
  int launch_fused(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, bool jser, FusedRun* r);
  void dump_device(const std::string& path, const void* src, size_t n);
  void print_fused_debug(const DecodePlan& p, const FusedRun& r, const uint32_t* hab, bool aborted);
  int finish_fused(const DecodePlan& p, FusedRun& r, clg_decoded* out, uint64_t* span_rec_base, bool* aborted,
                   bool* need_jser);
  // ---------------------------------------------------------------- small batches
  // A batch of at most kSmallBytes and clg::kZSmallTilesMax tiles, without Serializable
  // tables, decodes in ONE launch (k_decode_small_tiles, decode_fused.hip): the plan
  // goes up in one copy, and the kernel writes host outputs straight into pinned memory, so
  // the call is copy + launch + one wait -- the three-pass sequence is about 15 queue
  // operations, which for config 1 (44 logs, 73 KB) cost more than the decode.  A span that
  // goes wrong sends the batch down the usual path.  CLG_F_NO_SMALL_DECODE (or CLONOS_SMALL=0,
  // a developer switch) turns it off.
  static constexpr uint64_t kSmallBytes = 1u << 20;
  static constexpr uint32_t kSmallSpans = clg::kZSmallSpans;
  static constexpr uint64_t kSmallHostOut = 32u << 20;  // pinned output bytes at most (cap-sized)
  PinBuf h_small_out, h_small_res;
  // Decode errors kept on the fast path (FusedCtl::span_err; CLONOS_KEEP_ERRORS=0 turns it off,
  // a developer switch): a span whose error the full rules confirm keeps the fast run's records
  // before it, and only spans whose chains went wrong otherwise go to the robust pipeline.
  // Test switch (CLONOS_FUSED_PERTURB, FusedCtl::perturb): wrong chunk entries and a wrong
  // look-back result, which the checks must catch (k_decode_repair, run_small, emit).
  DevBuf d_zerr, d_sf_cls;
  DevBuf d_small;
  clg::SmallPlanArg small_arg;
  bool small_flip = false;
  bool small_ok(const DecodePlan& p, uint64_t log_bytes, const clg_decoded* out) const;
  static bool mapped_outputs(const clg_decoded& out, clg::DecodeOut* o);
  void host_tiles(DecodePlan& p);
  static uint32_t segtab_at(const DecodePlan& p, uint64_t i);
  bool small_handoffs_ok(const DecodePlan& p, const uint64_t* res);
  int run_small(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base, bool* aborted);
  int decode(const PlanBuild& build, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base,
             DecodePlan* prebuilt = nullptr);
  int plan_ok(const DecodePlan& p);

  // Per-span fallback after a fast run whose chains went wrong in some spans only (a
  // decode error, a record the fast rules cannot place): those spans are decoded together in
  // one robust run into scratch, their counts injected into the fast run's per-tile counts,
  // scan and emit re-run for the other spans (emit skips the bad ones), and the robust
  // records placed by one kernel (k_sf_place; their wide rows' record indices moved to the
  // batch's).  *done = false: not applicable (too many or too large bad spans), the
  // caller decodes the whole batch robustly.  The result equals the whole-batch robust
  // decode's: every span's records, the first error of the lowest span.
  // at most this many bad spans, and three quarters of the bytes: past that the whole batch
  // goes robust (one run either way; the fast run's second half is the saving)
  static constexpr uint32_t kSfMaxSpans = 8192;
  int span_fallback(DecodePlan& pf, const PlanBuild& build, uint64_t log_bytes, clg_decoded* out,
                    uint64_t* span_rec_base, bool* done);
  int after_abort(DecodePlan& pf, const PlanBuild& build, uint64_t log_bytes, clg_decoded* out,
                  uint64_t* span_rec_base, bool need_jser);

  // ---------------------------------------------------------------- asynchronous decode
  // clg_decode_logs_async: the three-pass decode is queued and the call returns; settle()
  // completes it (result, fallbacks) in clg_decode_wait or first thing in any other call
  // that needs the engine exclusively (see ENGINE_GUARD), so a pending decode never sees
  // its inputs change.  Slices into device memory on the gather stream and consumer seeks
  // leave it pending: they only read log segments and move consumer offsets.
  // Up to CLG_DECODE_MAX_INFLIGHT decodes are queued at once, each with its own slot (read-
  // back words, staged plan, completion event), so decode i+1's kernels are on the stream
  // before the host completes decode i and the GPU never waits for the host in between.
  // The device scratch (control words, bitmaps, tables) is shared and stream-ordered: the
  // fast path of decode i only needs its read-back.  A decode whose fast run aborted while a
  // later one was already queued has lost its scratch to that one, so it is decoded again
  // from its plan builder, and so are the later ones (rare: they may share its outputs).
  struct PendingDecode {
    bool active = false;  // queued on the GPU, not yet completed
    bool redo = false;    // its fast run's scratch is void: decode again when completed
    DecodePlan plan;
    FusedRun run;
    uint64_t log_bytes = 0;
    clg_decoded* out = nullptr;
    uint64_t* span_rec_base = nullptr;
    PlanBuild build;
    int status = CLG_OK;  // its result, for the clg_decode_wait that pairs with it
    std::string err;      // and its error text
    int64_t min_epoch = INT64_MIN;  // the smallest start epoch it decodes from (INT64_MIN: unknown)
  };
  // clg_truncate_all while decodes are queued (their ranges start at or above the checkpoint):
  // the segments it frees wait here until no decode is queued (the queued kernels may still
  // read them), and the logs' rebase generation tells a queued decode that re-plans (an abort's
  // fallback) to look its ranges up again
  std::vector<uint32_t> free_later;
  uint64_t rebase_gen = 0;
  int64_t q_min_epoch = INT64_MIN;  // clg_decode_logs_async -> decode_async: the call's smallest start epoch
  void release_later();
  std::deque<PendingDecode> pq;  // queued by clg_decode_logs_async, not yet waited for (oldest first)
  // the largest queued plan so far (the scratch is sized for it): a larger one is queued only
  // once nothing is in flight, since growing a buffer frees the one the GPU may still read
  uint64_t hw_tiles = 0, hw_spans = 0, hw_runs = 0, hw_segs = 0;
  bool hw_jser = false;
  bool any_active(size_t from = 0) const;
  int push_settled(int st, clg_decoded* out);
  // queued decodes' plans, recycled (a config-4 plan is ~4 MB: fresh pages cost page faults)
  std::vector<DecodePlan> plan_pool;
  int decode_async(PlanBuild build, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base,
                   DecodePlan* prebuilt = nullptr);
  bool slot_used(uint32_t slot) const;
  uint32_t free_slot() const;
  int settle(size_t upto = SIZE_MAX);
  int wait_oldest(std::string* err);
  int run_decode(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base);
  int run_decode_once(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base);
};

// Exclusive calls first complete a pending asynchronous decode (clg_decode_logs_async);
// ENGINE_GUARD_KEEP leaves it pending (calls that only read log segments on the gather
// stream or move consumer offsets).
#define ENGINE_GUARD_KEEP(e)                                        \
  if (!(e)) return fail(CLG_E_INVALID_ARG, "null engine");          \
  XGuard guard_((e)->mu)
#define ENGINE_GUARD(e) \
  ENGINE_GUARD_KEEP(e); \
  (e)->settle()

// A per-log call: only the log's stripe (see EngineLock).
struct LogGuard {
  std::mutex* s;
  LogGuard(clg_engine* e, uint32_t h) : s(e->mu.owned() ? nullptr : &e->mu.stripe[h % kLogStripes].m) {
    if (s) s->lock();
  }
  ~LogGuard() {
    if (s) s->unlock();
  }
};
#define LOG_GUARD(e, h)                                    \
  if (!(e)) return fail(CLG_E_INVALID_ARG, "null engine"); \
  LogGuard lguard_((e), (h))

// (What the typed-columns family's units share, the decodes into columns that replay preparation
// runs among it, is in engine_columns.h.)

#pragma GCC visibility pop
