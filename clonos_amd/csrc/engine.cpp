// engine.cpp -- host side of the MI355X causal-log engine (implements include/clonos_engine.h).
//
// Owns: the HBM segment pool (components of determinantBufferSize bytes), the per-log
// metadata with exactly the reference's semantics, host staging of appends, and the
// batching of all byte work into gfx950 kernels (kernels.hip) on one HIP stream.
//
// R/ = flink-runtime/src/main/java/org/apache/flink/runtime/causal/ of the reference.
// The log metadata mirrors R/log/thread/ThreadCausalLogImpl.java:51-527 line for line in
// behaviour (EpochStartOffset objects shared by reference with ConsumerOffset, Netty
// component-granular discardReadComponents), but the bytes never leave HBM.
//
// This unit: the error text, the registry of clg_host_register, engine create / destroy, timing,
// the segment pool, flush, append and upstream deltas, checkpoints and truncation, consumer
// seeks, jobs and log handles; and, until they have units of their own, the typed-columns
// family, replay preparation and the in-flight log.  Slices and digests are in
// engine_gather.cpp, the decodes in engine_decode.cpp; what the units share is in engine_impl.h.
#include "engine_impl.h"
#include "columns.h"
#include "encode_columns.h"
#include "pack.h"
#include "payload.h"
#include "placement.h"

static_assert(sizeof(clg_delta_req) == 32, "clg_delta_req layout");
static_assert(sizeof(clg_diff) == 24, "clg_diff layout");
static_assert(sizeof(clg_columns) == 232, "clg_columns layout");
static_assert(sizeof(clg_payloads) == 64, "clg_payloads layout");
static_assert(sizeof(clg_columns_in) == 176, "clg_columns_in layout");
static_assert(sizeof(clg_packed) == 136, "clg_packed layout");
static_assert(sizeof(clg_unpack_bad) == 16, "clg_unpack_bad layout");
static_assert(sizeof(clg_encoded) == 56, "clg_encoded layout");

namespace clg_internal {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// A launch helper's CLG_E_DEVICE carries the HIP error into the error text.
void note_launch_error(const char* what) {
  if (const char* m = clg::take_launch_error()) fail(CLG_E_DEVICE, "%s: %s", what, m);
}

}  // namespace clg_internal

// clg_host_register's ranges: host base -> device address (for CLG_MEM_MAPPED outputs)
namespace {
struct Mapped {
  uintptr_t host;
  uint64_t bytes;
  uintptr_t dev;
};
std::mutex g_map_mu;
std::vector<Mapped> g_mapped;
}  // namespace
// The device address of registered host memory [h, h + n) (0: not wholly inside one
// registered range).
uintptr_t clg_mapped_device_address(const void* h, uint64_t n) {
  std::lock_guard<std::mutex> g(g_map_mu);
  for (const Mapped& m : g_mapped)
    if (uintptr_t(h) >= m.host && uintptr_t(h) < m.host + m.bytes && n <= m.host + m.bytes - uintptr_t(h))
      return m.dev + (uintptr_t(h) - m.host);
  return 0;
}
// How many of the n bytes at h one copy may take: up to the first edge of a registered range
// inside them (the HIP runtime refuses a copy that crosses the end of registered memory).
uint64_t clg_mapped_piece(const void* h, uint64_t n) {
  std::lock_guard<std::mutex> g(g_map_mu);
  for (const Mapped& m : g_mapped)
    for (const uintptr_t edge : {m.host, m.host + uintptr_t(m.bytes)})
      if (edge > uintptr_t(h) && edge - uintptr_t(h) < n) n = edge - uintptr_t(h);
  return n;
}

namespace clg_internal {  // error text for the host-only translation units (response.cpp)
int set_error(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace clg_internal

// ---------------------------------------------------------------- timing helpers
hipEvent_t clg_engine::get_event() {
  if (!ev_pool.empty()) {
    hipEvent_t e = ev_pool.back();
    ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

// ready_only: only the timings whose end event has completed (the rest stay pending)
void clg_engine::collect_timings(bool ready_only) {
  if (ready_only) {
    std::vector<PendingTiming> later;
    for (auto& t : timings)
      if (hipEventQuery(t.b) == hipErrorNotReady) later.push_back(t);
    if (!later.empty()) {
      std::vector<PendingTiming> done;
      for (auto& t : timings)
        if (hipEventQuery(t.b) != hipErrorNotReady) done.push_back(t);
      timings.swap(done);
      collect_timings();
      timings.swap(later);
      return;
    }
  }
  for (auto& t : timings) {
    float ms = 0;
    hipEventSynchronize(t.b);
    hipEventElapsedTime(&ms, t.a, t.b);
    Stat& s = stats[t.name];
    s.launches++;
    s.ms += ms;
    s.bytes += t.bytes;
    ev_pool.push_back(t.a);
    ev_pool.push_back(t.b);
  }
  timings.clear();
}

int clg_engine::gwait() {
  if (g_pending) {
    g_pending = false;
    HIPCHK(hipStreamSynchronize(gstream));
  }
  return CLG_OK;
}

// The arena for kernels queued next on `stream`, its bump counter reset first.
int clg_engine::jarena_reset(clg::JArena* a) {
  CHK(d_jarena.ensure(jarena_bytes + 256));
  HIPCHK(hipMemsetAsync(d_jarena.p, 0, 8, stream));
  *a = clg::JArena{d_jarena.as<uint8_t>() + 256, jarena_bytes, d_jarena.as<unsigned long long>()};
  return CLG_OK;
}

// Queues a read-back of the arena's bump counter into slot k, after the walks queued so
// far; jarena_spilled(k) (after a sync) says whether any of them found the arena full --
// then some walk returned kJsSpill and whatever the kernels derived from it is void.
int clg_engine::jarena_note(int k) {
  CHK(h_jused.ensure(64));
  HIPCHK(hipMemcpyAsync(h_jused.as<uint64_t>() + k, d_jarena.p, 8, hipMemcpyDeviceToHost, stream));
  return CLG_OK;
}

int clg_engine::jarena_clear_note(int k) {
  CHK(h_jused.ensure(64));
  h_jused.as<uint64_t>()[k] = 0;
  return CLG_OK;
}

int clg_engine::jarena_grow() {
  CHK(sync());  // kernels still using the old arena
  if (jarena_bytes >= (size_t(1) << 36))
    return fail(CLG_E_DEVICE, "Serializable walker spill arena would exceed 64 GiB");
  jarena_bytes *= 2;
  stats["jser_arena_grow"].launches++;
  return CLG_OK;
}

int clg_engine::sync() {
  CHK(gwait());
  HIPCHK(hipStreamSynchronize(stream));
  collect_timings();
  return CLG_OK;
}

// notEnoughSpaceFor / addComponent (:351-353, :438-452): all-or-nothing.
int clg_engine::ensure_space(Log& l, int32_t n) {
  if (int64_t(l.writer) + n <= capacity(l)) return CLG_OK;
  std::lock_guard<std::mutex> g(pool_mu);
  return ensure_space_locked(l, n);
}

int clg_engine::ensure_space_locked(Log& l, int32_t n) {  // pool_mu held
  int64_t need_bytes = int64_t(l.writer) + n - capacity(l);
  if (need_bytes <= 0) return CLG_OK;
  size_t need = size_t((need_bytes + C() - 1) / C());
  if (need > free_segs.size())
    return fail(CLG_E_NOSPACE, "segment pool exhausted (need %zu, free %zu)", need, free_segs.size());
  for (size_t i = 0; i < need; ++i) {
    l.segs.push_back(free_segs.back());
    ++seg_life[free_segs.back()];
    free_segs.pop_back();
  }
  return CLG_OK;
}

void clg_engine::write_pending(Log& l, const uint8_t* b, uint32_t n) {
  if (l.flushed == l.writer && n) {
    std::lock_guard<std::mutex> g(dirty_mu);
    dirty.push_back(uint32_t(&l - logs.data()));
  }
  l.tail.insert(l.tail.end(), b, b + n);
  l.writer += int32_t(n);
}

// ---------------------------------------------------------------- flush (append scatter)
// Drops flushed bytes from the front of a log's host tail beyond the configured keep.
void clg_engine::trim_tail(Log& l) {
  const size_t keep = cfg.host_tail_bytes;
  const size_t flushed_in_tail = size_t(l.flushed - l.tail_start);
  if (flushed_in_tail <= 2 * keep) return;  // amortised: trim to `keep` once it doubled
  const size_t drop = flushed_in_tail - keep;
  l.tail.erase(l.tail.begin(), l.tail.begin() + long(drop));
  l.tail_start += int32_t(drop);
}

// Staged (unflushed) bytes of one log are bounded: past this the append that crossed it
// flushes (the host holds at most ~this + host_tail_bytes per log).
bool clg_engine::over_stage_limit(uint32_t h) const {
  const uint32_t lim = std::max<uint32_t>(65536u, 2u * cfg.host_tail_bytes);
  return h < logs.size() && logs[h].open && logs[h].pending_bytes() > lim;
}

int clg_engine::flush() {
  size_t total = 0, nchunks = 0;
  for (uint32_t h : dirty) {
    const Log& l = logs[h];
    if (l.open && l.pending_bytes()) {
      total += l.pending_bytes();
      nchunks += l.pending_bytes() / C() + 2;
    }
  }
  if (total == 0) {
    dirty.clear();
    return CLG_OK;
  }
  CHK(gwait());  // an in-flight gather may still read the segments about to be written
  const size_t desc_bytes = nchunks * sizeof(clg::ScatterChunk);
  CHK(h_stage.ensure(total));
  CHK(h_desc.ensure(desc_bytes));
  CHK(d_stage.ensure(total));
  CHK(d_desc.ensure(desc_bytes));
  uint8_t* hs = h_stage.as<uint8_t>();
  clg::ScatterChunk* ch = h_desc.as<clg::ScatterChunk>();
  size_t off = 0, n = 0;
  for (uint32_t h : dirty) {
    Log& l = logs[h];
    const uint32_t pb = l.open ? l.pending_bytes() : 0u;
    if (!pb) continue;
    memcpy(hs + off, l.pending_data(), pb);
    int32_t p = l.flushed;
    size_t src = off;
    size_t left = pb;
    while (left) {
      const uint32_t si = uint32_t(p) / C(), so = uint32_t(p) % C();
      const uint32_t take = uint32_t(std::min<size_t>(left, C() - so));
      ch[n++] = clg::ScatterChunk{seg_addr(l.segs[si]) + so, src, take, life_word(l.segs[si], left > take)};
      p += int32_t(take);
      src += take;
      left -= take;
    }
    off += pb;
    l.flushed = l.writer;
    trim_tail(l);
  }
  dirty.clear();
  HIPCHK(hipMemcpyAsync(d_stage.p, hs, total, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_desc.p, ch, n * sizeof(clg::ScatterChunk), hipMemcpyHostToDevice, stream));
  CHK(timed("append_scatter", 2 * total, [&] {
    return clg::launch_scatter(d_desc.as<clg::ScatterChunk>(), uint32_t(n), d_stage.as<uint8_t>(), stream, side_arg());
  }));
  // the pinned staging buffers are reused by the next flush: wait for the copies
  HIPCHK(hipStreamSynchronize(stream));
  return CLG_OK;
}

// ---------------------------------------------------------------- ThreadCausalLog ops
int clg_engine::append(uint32_t h, int64_t epoch, const uint8_t* b, uint32_t n) {  // :158-177
  Log* l;
  CHK(get_log(h, &l));
  if (l->depth == 0) return CLG_OK;
  if (n && !b) return fail(CLG_E_INVALID_ARG, "null record");
  CHK(ensure_space(*l, int32_t(n)));
  compute_if_absent(*l, epoch);
  write_pending(*l, b, n);
  return CLG_OK;
}

int clg_engine::upstream(uint32_t h, int64_t epoch, int32_t off_from_epoch, const uint8_t* d, uint32_t n) {  // :117-154
  Log* l;
  CHK(get_log(h, &l));
  if (n == 0) return CLG_OK;
  if (!d) return fail(CLG_E_INVALID_ARG, "null delta");
  auto es = compute_if_absent(*l, epoch);
  const int32_t cur = l->writer - es->offset;
  const int32_t num_new = (off_from_epoch + int32_t(n)) - cur;
  if (num_new > 0) {
    // :136-137 add components before delta.readerIndex(<0) throws (:143): capacity grows
    CHK(ensure_space(*l, num_new));
    if (num_new > int32_t(n))
      return fail(CLG_E_GAP, "upstream delta leaves a gap: offsetFromEpoch %d, %u bytes, log at %d", off_from_epoch,
                  n, cur);
    write_pending(*l, d + (n - uint32_t(num_new)), uint32_t(num_new));
  }
  return CLG_OK;
}

// Batched processUpstreamDelta (:117-154) over one input buffer.  Device input (e.g.
// an RCCL receive buffer) is scattered straight into the log segments: pending host
// bytes are flushed first, so the logs' byte order is preserved.
int clg_engine::upstream_batch(clg_delta_req* r, uint32_t n, const uint8_t* bytes, uint32_t in_kind) {
  HostTimer ht(this, "host_upstream_batch");
  if (in_kind != CLG_MEM_DEVICE) {
    for (uint32_t i = 0; i < n; ++i) {
      r[i].status = upstream(r[i].log, r[i].epoch, r[i].offset_from_epoch, bytes + r[i].src_off, r[i].len);
    }
    return CLG_OK;
  }
  std::optional<HostTimer> hsub(std::in_place, this, "host_up_wait");  // (CLONOS_HOST_PROF sub-stages)
  CHK(flush());
  CHK(gwait());  // the scatter below writes segments an in-flight gather may read
  hsub.reset();
  if (n >= kParallelLogs) {
    int st = CLG_OK;
    if (upstream_parallel(r, n, bytes, &st)) return st;
  }
  // the chunks go straight into the pinned descriptor buffer (a config-4 batch has 66 k of
  // them: a fresh vector per call cost page faults, and a copy)
  size_t bound = 0;
  for (uint32_t i = 0; i < n; ++i) bound += r[i].len / C() + 2;
  CHK(h_desc.ensure(std::max<size_t>(1, bound) * sizeof(clg::ScatterChunk)));
  clg::ScatterChunk* ch = h_desc.as<clg::ScatterChunk>();
  size_t nch = 0, total = 0;
  std::unique_lock<std::mutex> pool_guard(pool_mu);  // once for the batch, not per log
  for (uint32_t i = 0; i < n; ++i) {
    r[i].status = CLG_OK;
    Log* l;
    if ((r[i].status = get_log(r[i].log, &l)) != CLG_OK || r[i].len == 0) continue;
    auto es = compute_if_absent(*l, r[i].epoch);
    const int32_t cur = l->writer - es->offset;
    const int32_t num_new = (r[i].offset_from_epoch + int32_t(r[i].len)) - cur;
    if (num_new <= 0) continue;
    if ((r[i].status = ensure_space_locked(*l, num_new)) != CLG_OK) continue;  // before the gap check (:136-143)
    if (num_new > int32_t(r[i].len)) {
      r[i].status = fail(CLG_E_GAP, "upstream delta leaves a gap: offsetFromEpoch %d, %u bytes, log at %d",
                         r[i].offset_from_epoch, r[i].len, cur);
      continue;
    }
    int32_t p = l->writer;
    uint64_t src = r[i].src_off + (r[i].len - uint32_t(num_new));
    uint32_t left = uint32_t(num_new);
    while (left) {
      const uint32_t si = uint32_t(p) / C(), so = uint32_t(p) % C();
      const uint32_t take = std::min<uint32_t>(left, C() - so);
      ch[nch++] = clg::ScatterChunk{seg_addr(l->segs[si]) + so, src, take, life_word(l->segs[si], left > take)};
      p += int32_t(take);
      src += take;
      left -= take;
    }
    l->writer += num_new;
    l->flushed = l->writer;
    reset_tail(*l);  // these bytes go to HBM only
    total += size_t(num_new);
  }
  pool_guard.unlock();
  if (!nch) return CLG_OK;
  const size_t db = nch * sizeof(clg::ScatterChunk);
  CHK(d_desc.ensure(db));
  HIPCHK(hipMemcpyAsync(d_desc.p, h_desc.p, db, hipMemcpyHostToDevice, stream));
  CHK(timed("upstream_scatter", 2 * total, [&] {
    return clg::launch_scatter(d_desc.as<clg::ScatterChunk>(), uint32_t(nch), bytes, stream, side_arg());
  }));
  return sync();  // the caller's buffer and the pinned descriptors are free again
}

bool clg_engine::upstream_parallel(clg_delta_req* r, uint32_t n, const uint8_t* bytes, int* out_st) {
  std::optional<HostTimer> hsub(std::in_place, this, "host_up_seen");
  up_seen.assign(logs.size(), 0);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t h = r[i].log;
    if (h < logs.size()) {
      if (up_seen[h]) return false;  // two deltas of one log apply in order: the serial loop
      up_seen[h] = 1;
    }
  }
  WorkPool* wp = workers();
  const unsigned P = wp->size();
  const uint32_t per = (n + P - 1) / P, Cb = C();
  up_plan.resize(n);
  // per part: segments, chunks and bytes it needs, and whether a request leaves a gap
  struct UpPart {
    uint64_t need = 0, chunks = 0, bytes = 0;
    bool gap = false;
  };
  std::vector<UpPart> upart(P + 1);
  hsub.emplace(this, "host_up_pass1");
  wp->run([&](unsigned k, unsigned) {
    UpPart q;
    for (uint32_t i = k * per; i < std::min(n, (k + 1) * per); ++i) {
      UpPlan& u = up_plan[i];
      u = UpPlan{0, 0, 0, 0, 0, 0, 0};
      r[i].status = CLG_OK;
      Log* l;
      if ((r[i].status = get_log(r[i].log, &l)) != CLG_OK || r[i].len == 0) continue;
      auto es = compute_if_absent(*l, r[i].epoch);
      const int32_t cur = l->writer - es->offset;
      const int32_t num_new = (r[i].offset_from_epoch + int32_t(r[i].len)) - cur;
      if (num_new <= 0) continue;
      const int64_t need_bytes = int64_t(l->writer) + num_new - capacity(*l);
      u.num_new = num_new;
      u.writer = l->writer;
      u.cur = cur;
      u.need = need_bytes > 0 ? uint32_t((need_bytes + Cb - 1) / Cb) : 0u;
      q.need += u.need;
      if (num_new > int32_t(r[i].len)) {
        q.gap = true;
      } else {
        const uint32_t p = uint32_t(u.writer);
        u.chunks = (p + uint32_t(num_new) - 1) / Cb - p / Cb + 1;
        q.chunks += u.chunks;
        q.bytes += uint64_t(num_new);
      }
    }
    upart[k + 1] = q;
  });
  hsub.emplace(this, "host_up_serial");
  std::unique_lock<std::mutex> pool_guard(pool_mu);
  const size_t top = free_segs.size();
  size_t taken = 0, nch = 0, total = 0;
  bool any_gap = false;
  for (unsigned k = 0; k < P; ++k) {
    any_gap |= upart[k + 1].gap;
    upart[k + 1].need += upart[k].need;
    upart[k + 1].chunks += upart[k].chunks;
    upart[k + 1].bytes += upart[k].bytes;
  }
  // every request served (the usual batch): each part places its own segments and chunks
  // from the parts' prefix in the second pass, as the request-order loop below would
  const bool placed_in_parts = !any_gap && upart[P].need <= top;
  if (placed_in_parts) {
    taken = upart[P].need;
    nch = upart[P].chunks;
    total = upart[P].bytes;
  } else for (uint32_t i = 0; i < n; ++i) {  // request order: the pool and the chunk list
    UpPlan& u = up_plan[i];
    if (!u.num_new) continue;
    if (u.need > top - taken) {
      r[i].status = fail(CLG_E_NOSPACE, "segment pool exhausted (need %u, free %zu)", u.need, top - taken);
      u.num_new = 0;
      u.need = 0;
      continue;
    }
    u.seg_from = taken;
    taken += u.need;
    if (u.num_new > int32_t(r[i].len)) {  // the segments stay (:136-143), nothing is written
      r[i].status = fail(CLG_E_GAP, "upstream delta leaves a gap: offsetFromEpoch %d, %u bytes, log at %d",
                         r[i].offset_from_epoch, r[i].len, u.cur);
      u.num_new = 0;
      continue;
    }
    u.ch_from = nch;  // (u.chunks from the first pass: no log record touched here)
    nch += u.chunks;
    total += size_t(u.num_new);
  }
  if (int st = h_desc.ensure(std::max<size_t>(1, nch) * sizeof(clg::ScatterChunk)); st != CLG_OK) {
    *out_st = st;
    return true;
  }
  clg::ScatterChunk* ch = h_desc.as<clg::ScatterChunk>();
  hsub.emplace(this, "host_up_pass2");
  wp->run([&](unsigned k, unsigned) {
    uint64_t sf = upart[k].need, cf = upart[k].chunks;
    for (uint32_t i = k * per; i < std::min(n, (k + 1) * per); ++i) {
      UpPlan& u = up_plan[i];
      if (placed_in_parts && u.num_new) {
        u.seg_from = sf;
        sf += u.need;
        u.ch_from = cf;
        cf += u.chunks;
      }
      if (!u.need && !u.num_new) continue;
      Log& l = logs[r[i].log];
      for (uint32_t j = 0; j < u.need; ++j) {  // pop order
        const uint32_t sg = free_segs[top - 1 - (u.seg_from + j)];
        l.segs.push_back(sg);
        ++seg_life[sg];  // (each segment is taken by one part)
      }
      if (!u.num_new) continue;
      int32_t p = l.writer;
      uint64_t src = r[i].src_off + (r[i].len - uint32_t(u.num_new));
      uint32_t left = uint32_t(u.num_new);
      uint64_t c = u.ch_from;
      while (left) {
        const uint32_t si = uint32_t(p) / Cb, so = uint32_t(p) % Cb;
        const uint32_t take = std::min<uint32_t>(left, Cb - so);
        ch[c++] = clg::ScatterChunk{seg_addr(l.segs[si]) + so, src, take, life_word(l.segs[si], left > take)};
        p += int32_t(take);
        src += take;
        left -= take;
      }
      l.writer += u.num_new;
      l.flushed = l.writer;
      reset_tail(l);  // these bytes go to HBM only
    }
  });
  free_segs.resize(top - taken);
  pool_guard.unlock();
  hsub.emplace(this, "host_up_gpu");
  *out_st = CLG_OK;
  if (!nch) return true;
  const size_t db = nch * sizeof(clg::ScatterChunk);
  if ((*out_st = d_desc.ensure(db)) != CLG_OK) return true;
  if (hipMemcpyAsync(d_desc.p, h_desc.p, db, hipMemcpyHostToDevice, stream) != hipSuccess) {
    *out_st = fail(CLG_E_DEVICE, "hipMemcpyAsync failed");
    return true;
  }
  if ((*out_st = timed("upstream_scatter", 2 * total, [&] {
         return clg::launch_scatter(d_desc.as<clg::ScatterChunk>(), uint32_t(nch), bytes, stream, side_arg());
       })) != CLG_OK)
    return true;
  *out_st = sync();
  return true;
}

int clg_engine::has_delta(uint32_t h, ChKey k, int64_t epoch, int32_t* out) {  // :196-240
  Log* l;
  CHK(get_log(h, &l));
  *out = 0;
  if (l->depth == 0) return CLG_OK;
  auto it = l->epochs.find(epoch);
  if (it == l->epochs.end()) return CLG_OK;
  auto ci = l->consumers.find(k);
  if (ci == l->consumers.end()) ci = l->consumers.emplace(k, Consumer{EpochMap::ref(*it), 0}).first;
  Consumer& c = ci->second;
  if (c.es->id != epoch) {
    if (c.es->id > epoch)
      return fail(CLG_E_CONSUMER_BACKWARDS, "Consumer went backwards, current epoch %lld requested %lld",
                  (long long)c.es->id, (long long)epoch);
    c.es = EpochMap::ref(*it);
    c.offset = 0;
  }
  *out = bytes_to_send(*l, epoch, c.es->offset + c.offset) != 0;
  return CLG_OK;
}

int clg_engine::offset_from_epoch(uint32_t h, ChKey k, int32_t* out) {  // :243-246
  Log* l;
  CHK(get_log(h, &l));
  auto ci = l->consumers.find(k);
  if (ci == l->consumers.end()) return fail(CLG_E_NO_CONSUMER, "consumer not registered on log %u", h);
  *out = ci->second.offset;
  return CLG_OK;
}

// getDeltaForConsumer :249-277, metadata half: returns (phys, nb) and advances.
int clg_engine::take_delta(uint32_t h, ChKey k, int64_t epoch, int32_t* phys, int32_t* nb) {
  Log* l;
  CHK(get_log(h, &l));
  auto ci = l->consumers.find(k);
  if (ci == l->consumers.end()) return fail(CLG_E_NO_CONSUMER, "consumer not registered on log %u", h);
  Consumer& c = ci->second;
  const int32_t p = c.es->offset + c.offset;
  const int32_t n = bytes_to_send(*l, epoch, p);
  if (n < 0 || p < 0 || int64_t(p) + n > capacity(*l))
    return fail(CLG_E_STATE, "delta [%d, %d) outside log of capacity %d", p, p + n, capacity(*l));
  c.offset += n;
  *phys = p;
  *nb = n;
  return CLG_OK;
}

// notifyCheckpointComplete :398-435 (flushes first so no staged byte lives in a dropped
// component).
int clg_engine::checkpoint_complete(Log& l, int64_t cp) { return checkpoint_complete(l, cp, free_segs); }

// (freed: where the dropped segments go -- a host thread's own list in the parallel truncation)
int clg_engine::checkpoint_complete(Log& l, int64_t cp, std::vector<uint32_t>& freed) {
  const int32_t R = compute_if_absent(l, cp)->offset;  // (read before the erase moves entries)
  l.epochs.erase_below(cp);
  if (R < 0 || R > l.writer) return fail(CLG_E_STATE, "readerIndex %d outside [0, %d]", R, l.writer);
  int32_t move = 0;
  if (R != 0) {
    size_t drop;
    if (R == l.writer && l.writer == capacity(l)) {  // discard-all case
      drop = l.segs.size();
      move = R;
    } else {
      drop = size_t(R) / C();
      move = int32_t(drop * C());
    }
    for (size_t i = 0; i < drop; ++i) freed.push_back(l.segs[i]);
    l.segs.erase_front(drop);
  }
  l.epochs.rebase(move);
  l.writer -= move;
  l.flushed -= move;
  l.tail_start -= move;
  if (l.tail_start < 0) {  // bytes of dropped components
    l.tail.erase(l.tail.begin(), l.tail.begin() + std::min<long>(long(l.tail.size()), long(-l.tail_start)));
    l.tail_start = 0;
    if (l.tail_start + int32_t(l.tail.size()) != l.writer) reset_tail(l);
  }
  return CLG_OK;
}

// The CPUs this process may use: its affinity mask, capped by a cgroup CPU quota (a GPU box
// shares its host between GPUs: 16 CPUs per GPU on the MI355X pool).
int clg_engine::usable_cpus() {
  int n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  if (n <= 0) n = int(std::thread::hardware_concurrency());
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long period = 0;
    if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
      n = std::min<long long>(n, std::max<long long>(1, atoll(q) / period));
    fclose(f);
  }
  return std::max(1, n);
}

// Host threads for the per-log loops: CLONOS_HOST_THREADS, else up to 16 of the usable CPUs.
// Config 4's step on one box (round 5): 2.49 ms with 16 against 3.1-3.4 ms with 8; round 6,
// median of four each: 2.09 / 2.20 / 2.40 ms with 16 / 14 / 12.
WorkPool* clg_engine::workers() {
  if (!host_pool) {
    const int n = std::max(1, std::min(sw.host_threads, usable_cpus()));
    host_pool = std::make_unique<WorkPool>(unsigned(n));
  }
  return host_pool.get();
}

// =======================================================================================
// C-ABI
// =======================================================================================

extern "C" {

void clg_config_default(clg_config* cfg) {
  memset(cfg, 0, sizeof *cfg);
  cfg->segment_bytes = 16384;  // NettyConfig.java:86-89
  cfg->pool_segments = 16384;  // 256 MiB
  cfg->device = 0;
  cfg->sharing_depth = CLG_FULL_SHARING;
  cfg->host_tail_bytes = 16384;    // one component of each log's tail kept on the host
  cfg->ifl_segment_bytes = 32768;  // the in-flight log's pool: Flink's 32 KiB memory segments
  cfg->ifl_pool_segments = 4096;   // 128 MiB
}

int clg_abi_version(void) { return CLG_ABI_VERSION; }

int clg_host_register(void* p, uint64_t bytes) {
  if (!p || !bytes) return fail(CLG_E_INVALID_ARG, "null or empty range");
  hipError_t er = hipHostRegister(p, size_t(bytes), hipHostRegisterMapped);
  if (er != hipSuccess) return fail(CLG_E_DEVICE, "hipHostRegister(%llu bytes): %s", (unsigned long long)bytes,
                                     hipGetErrorString(er));
  void* d = nullptr;
  er = hipHostGetDevicePointer(&d, p, 0);
  if (er != hipSuccess) {
    (void)hipHostUnregister(p);
    return fail(CLG_E_DEVICE, "hipHostGetDevicePointer: %s", hipGetErrorString(er));
  }
  std::lock_guard<std::mutex> g(g_map_mu);
  g_mapped.push_back(Mapped{uintptr_t(p), bytes, uintptr_t(d)});
  return CLG_OK;
}

int clg_host_unregister(void* p) {
  {
    std::lock_guard<std::mutex> g(g_map_mu);
    auto it = std::find_if(g_mapped.begin(), g_mapped.end(), [&](const Mapped& m) { return m.host == uintptr_t(p); });
    if (it == g_mapped.end()) return fail(CLG_E_INVALID_ARG, "range not registered");
    g_mapped.erase(it);
  }
  const hipError_t er = hipHostUnregister(p);
  return er == hipSuccess ? CLG_OK : fail(CLG_E_DEVICE, "hipHostUnregister: %s", hipGetErrorString(er));
}

const char* clg_last_error(void) { return g_err.c_str(); }

int clg_engine_create(const clg_config* cfg, clg_engine** out) {
  if (!cfg || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->segment_bytes < 16 || (cfg->segment_bytes & 15) || cfg->pool_segments == 0)
    return fail(CLG_E_INVALID_ARG, "segment_bytes must be a positive multiple of 16 and pool_segments > 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(CLG_E_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(CLG_E_INVALID_ARG, "device %d out of range", cfg->device);
  std::unique_ptr<clg_engine> e(new clg_engine());
  e->cfg = *cfg;
  e->fused_decode = !(cfg->flags & CLG_F_ROBUST_DECODE) && !e->sw.robust_decode;
  e->small_decode = !(cfg->flags & CLG_F_NO_SMALL_DECODE) && e->sw.small_decode;
  if (e->sw.jser_arena) e->jarena_bytes = e->sw.jser_arena;
  HIPCHK(hipSetDevice(cfg->device));
  {
    // The device-output slice gather (HBM-bound) runs beside the next decode (VALU-bound):
    // its queue gets the higher priority so its workgroups are dispatched first
    // (CLONOS_GATHER_PRIO=0: same priority as the decode stream; 2: the decode stream's
    // queue higher instead, so the decode's short set-up, scan and read-back launches do not
    // wait behind the gather's workgroups).
    const int mode = e->sw.gather_prio;
    int lo = 0, hi = 0;
    const bool prio = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo;
    if (prio && mode == 2) HIPCHK(hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, hi));
    else HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    if (prio && mode == 1) HIPCHK(hipStreamCreateWithPriority(&e->gstream, hipStreamNonBlocking, hi));
    else HIPCHK(hipStreamCreateWithFlags(&e->gstream, hipStreamNonBlocking));
  }
  HIPCHK(hipEventCreateWithFlags(&e->gready, hipEventDisableTiming));
  const size_t pool_bytes = size_t(cfg->segment_bytes) * cfg->pool_segments;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, pool_bytes + 2 * kPoolGuard));  // guards: aligned over-reads either side
  e->pool_alloc = p;
  e->pool = static_cast<uint8_t*>(p) + kPoolGuard;
  e->free_segs.resize(cfg->pool_segments);
  for (uint32_t i = 0; i < cfg->pool_segments; ++i) e->free_segs[i] = cfg->pool_segments - 1 - i;
  e->seg_life.assign(cfg->pool_segments, 0u);
  // the sidecar: C / 64 entries per segment (256 for 16 KiB: config 3 averages ~100), its
  // positions 16 bits (segments up to 64 KiB); CLONOS_SIDECAR=0 turns it off (developer A/B)
  if (cfg->segment_bytes <= 65536u && cfg->pool_segments && e->sw.sidecar) {
    const uint32_t cap = std::min<uint32_t>(clg::kSideCapMax, std::max<uint32_t>(8u, cfg->segment_bytes / 64u));
    const size_t hb = size_t(cfg->pool_segments) * 8, eb = size_t(cfg->pool_segments) * cap * 4;
    // (no room beside a pool sized to the HBM: the engine runs without it, the decode scans)
    if (hipMalloc(&p, hb + eb) == hipSuccess) {
      e->side_alloc = p;
      HIPCHK(hipMemset(p, 0, hb));  // life 0: every segment's first chunk starts its list
      e->side = clg::SideCar{static_cast<uint64_t*>(p), reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(p) + hb),
                             e->pool, pool_bytes, cfg->segment_bytes, cap};
    } else {
      (void)hipGetLastError();  // (the failed allocation is not the engine's error)
    }
  }
  e->ifl_C = cfg->ifl_segment_bytes ? cfg->ifl_segment_bytes : 32768u;
  const uint32_t ifl_n = cfg->ifl_pool_segments ? cfg->ifl_pool_segments : 4096u;
  if (e->ifl_C % 16) return fail(CLG_E_INVALID_ARG, "ifl_segment_bytes must be a multiple of 16");
  e->cfg.ifl_segment_bytes = e->ifl_C;
  e->cfg.ifl_pool_segments = ifl_n;
  HIPCHK(hipMalloc(&p, size_t(e->ifl_C) * ifl_n + 2 * kPoolGuard));
  e->ifl_alloc = p;
  e->ifl_pool = static_cast<uint8_t*>(p) + kPoolGuard;
  e->ifl_free.resize(ifl_n);
  for (uint32_t i = 0; i < ifl_n; ++i) e->ifl_free[i] = ifl_n - 1 - i;
  e->jobs.emplace_back();  // job 0: the default job
  e->jobs[0].open = true;
  e->jobs[0].depth = cfg->sharing_depth;
  *out = e.release();
  return CLG_OK;
}

void clg_engine_destroy(clg_engine* e) {
  if (!e) return;
  hipSetDevice(e->cfg.device);
  e->settle();  // a pending asynchronous decode: its events go back to the pool
  hipStreamSynchronize(e->stream);
  e->gwait();
  for (auto& t : e->timings) {
    hipEventDestroy(t.a);
    hipEventDestroy(t.b);
  }
  for (auto ev : e->ev_pool) hipEventDestroy(ev);
  for (auto ev : e->zdone)
    if (ev) hipEventDestroy(ev);
  if (e->pool_alloc) hipFree(e->pool_alloc);
  if (e->side_alloc) hipFree(e->side_alloc);
  if (e->ifl_alloc) hipFree(e->ifl_alloc);
  hipStreamDestroy(e->stream);
  if (e->gstream) hipStreamDestroy(e->gstream);
  if (e->gready) hipEventDestroy(e->gready);
  for (auto ev : e->gdone)
    if (ev) hipEventDestroy(ev);
  delete e;
}

void* clg_engine_stream(clg_engine* e) { return e ? (void*)e->stream : nullptr; }
void* clg_gather_stream(clg_engine* e) { return e ? (void*)e->gstream : nullptr; }

int clg_sync(clg_engine* e) {
  ENGINE_GUARD(e);
  CHK(e->flush());
  return e->sync();
}

int clg_pool_stats(clg_engine* e, uint32_t* used, uint32_t* free_segments) {
  ENGINE_GUARD(e);
  *free_segments = uint32_t(e->free_segs.size());
  *used = e->cfg.pool_segments - *free_segments;
  return CLG_OK;
}

int clg_job_open(clg_engine* e, uint64_t job_lo, uint64_t job_hi, int32_t sharing_depth, uint32_t* job) {
  ENGINE_GUARD(e);
  if (!job) return fail(CLG_E_INVALID_ARG, "null argument");
  for (uint32_t j = 0; j < e->jobs.size(); ++j)
    if (e->jobs[j].open && e->jobs[j].lo == job_lo && e->jobs[j].hi == job_hi && j != 0)
      return fail(CLG_E_INVALID_ARG, "job already open");
  Job nj;
  nj.open = true;
  nj.lo = job_lo;
  nj.hi = job_hi;
  nj.depth = sharing_depth;
  for (uint32_t j = 1; j < e->jobs.size(); ++j)
    if (!e->jobs[j].open) {
      e->jobs[j] = nj;
      *job = j;
      return CLG_OK;
    }
  e->jobs.push_back(nj);
  *job = uint32_t(e->jobs.size() - 1);
  return CLG_OK;
}

int clg_job_close(clg_engine* e, uint32_t job) {
  ENGINE_GUARD(e);
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  for (uint32_t h = 0; h < e->logs.size(); ++h)
    if (e->logs[h].open && e->logs[h].job == job) CHK(clg_log_close(e, h));
  if (job != 0) e->jobs[job] = Job();
  else e->jobs[0].latest_cp = 0;
  return CLG_OK;
}

int clg_ifl_pool_stats(clg_engine* e, uint32_t* used, uint32_t* free_segments) {
  ENGINE_GUARD(e);
  *free_segments = uint32_t(e->ifl_free.size());
  *used = e->cfg.ifl_pool_segments - *free_segments;
  return CLG_OK;
}

int clg_log_open(clg_engine* e, uint32_t job, const clg_causal_log_id* id, uint32_t* handle) {
  ENGINE_GUARD(e);
  if (!id || !handle) return fail(CLG_E_INVALID_ARG, "null argument");
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  const IdKey k = key_of(job, *id);
  if (e->by_id.count(k)) return fail(CLG_E_INVALID_ARG, "log already open");
  Log l;
  l.id = *id;
  l.job = job;
  l.depth = e->jobs[job].depth;
  l.open = true;
  if (e->free_segs.empty()) return fail(CLG_E_NOSPACE, "segment pool exhausted");
  l.segs.push_back(e->free_segs.back());  // ctor addComponent() :102
  ++e->seg_life[e->free_segs.back()];
  e->free_segs.pop_back();
  const uint32_t h = uint32_t(e->logs.size());  // handles are never reused: a stale one is CLG_E_NO_LOG
  e->logs.push_back(std::move(l));
  e->by_id[k] = h;
  *handle = h;
  return CLG_OK;
}

int clg_log_close(clg_engine* e, uint32_t h) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  CHK(e->sync());
  for (uint32_t s : l->segs) e->free_segs.push_back(s);
  e->by_id.erase(key_of(l->job, l->id));
  *l = Log();
  return CLG_OK;
}

int clg_log_find(clg_engine* e, uint32_t job, const clg_causal_log_id* id, uint32_t* handle) {
  ENGINE_GUARD(e);
  auto it = e->by_id.find(key_of(job, *id));
  if (it == e->by_id.end()) return fail(CLG_E_NO_LOG, "log not found");
  *handle = it->second;
  return CLG_OK;
}

int clg_log_get_id(clg_engine* e, uint32_t h, clg_causal_log_id* id, uint32_t* job) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  if (id) *id = l->id;
  if (job) *job = l->job;
  return CLG_OK;
}

int clg_append(clg_engine* e, uint32_t log, int64_t epoch, const uint8_t* rec, uint32_t n) {
  bool spill;
  {
    LOG_GUARD(e, log);
    CHK(e->append(log, epoch, rec, n));
    spill = e->over_stage_limit(log);
  }
  if (!spill) return CLG_OK;
  ENGINE_GUARD(e);  // bounded write-behind: this log's staged bytes go to HBM now
  return e->flush();
}

int clg_append_batch(clg_engine* e, const uint32_t* log, const int64_t* epoch, const uint64_t* off,
                     const uint32_t* len, uint32_t n, const uint8_t* bytes) {
  ENGINE_GUARD(e);
  for (uint32_t i = 0; i < n; ++i) CHK(e->append(log[i], epoch[i], bytes + off[i], len[i]));
  return CLG_OK;
}

int clg_upstream_delta(clg_engine* e, uint32_t log, int64_t epoch, int32_t off, const uint8_t* d, uint32_t n) {
  bool spill;
  {
    LOG_GUARD(e, log);
    CHK(e->upstream(log, epoch, off, d, n));
    spill = e->over_stage_limit(log);
  }
  if (!spill) return CLG_OK;
  ENGINE_GUARD(e);
  return e->flush();
}

int clg_log_length(clg_engine* e, uint32_t h, int32_t* out) {  // :180-192
  LOG_GUARD(e, h);
  Log* l;
  CHK(e->get_log(h, &l));
  *out = l->epochs.empty() ? l->writer : l->writer - l->epochs.begin()->offset;
  return CLG_OK;
}

int clg_log_length_batch(clg_engine* e, const uint32_t* log, uint32_t n, int32_t* out, uint64_t* total) {
  ENGINE_GUARD(e);
  if (n && !log) return fail(CLG_E_INVALID_ARG, "null argument");
  uint64_t t = 0;
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(e->get_log(log[i], &l));
    const int32_t v = l->epochs.empty() ? l->writer : l->writer - l->epochs.begin()->offset;
    if (out) out[i] = v;
    t += uint64_t(v);
  }
  if (total) *total = t;
  return CLG_OK;
}

int clg_has_delta(clg_engine* e, uint32_t log, clg_channel_id c, int64_t epoch, int32_t* out) {
  LOG_GUARD(e, log);
  return e->has_delta(log, ChKey{c.lo, c.hi}, epoch, out);
}

int clg_offset_from_epoch(clg_engine* e, uint32_t log, clg_channel_id c, int32_t* out) {
  LOG_GUARD(e, log);
  return e->offset_from_epoch(log, ChKey{c.lo, c.hi}, out);
}

}  // extern "C"

extern "C" {

int clg_notify_checkpoint_complete(clg_engine* e, uint32_t h, int64_t cp) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  CHK(e->flush());
  return e->checkpoint_complete(*l, cp);
}

int clg_unregister_consumer(clg_engine* e, uint32_t h, clg_channel_id c) {
  LOG_GUARD(e, h);
  Log* l;
  CHK(e->get_log(h, &l));
  l->consumers.erase(ChKey{c.lo, c.hi});
  return CLG_OK;
}

int clg_log_get_state(clg_engine* e, uint32_t h, clg_log_state* st, int64_t* ids, int32_t* offs, int32_t cap) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  st->writer = l->writer;
  st->capacity = e->capacity(*l);
  st->n_components = int32_t(l->segs.size());
  st->n_epochs = int32_t(l->epochs.size());
  int32_t i = 0;
  for (auto& ep : l->epochs) {
    if (i < cap) {
      if (ids) ids[i] = ep.id;
      if (offs) offs[i] = ep.offset;
    }
    ++i;
  }
  return i > cap && (ids || offs) ? fail(CLG_E_CAPACITY, "%d epochs", i) : CLG_OK;
}

int clg_consumer_state(clg_engine* e, uint32_t h, clg_channel_id c, int32_t* exists, int64_t* epoch, int32_t* offset) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  auto ci = l->consumers.find(ChKey{c.lo, c.hi});
  *exists = ci != l->consumers.end();
  if (*exists) {
    *epoch = ci->second.es->id;
    *offset = ci->second.offset;
  }
  return CLG_OK;
}

}  // extern "C"

extern "C" {

int clg_consumer_seek(clg_engine* e, uint32_t h, clg_channel_id c, int64_t epoch, int32_t offset) {
  ENGINE_GUARD_KEEP(e);
  Log* l;
  CHK(e->get_log(h, &l));
  auto it = l->epochs.find(epoch);
  if (it == l->epochs.end()) return fail(CLG_E_STATE, "epoch %lld not in log", (long long)epoch);
  l->consumers[ChKey{c.lo, c.hi}] = Consumer{EpochMap::ref(*it), offset};
  return CLG_OK;
}

int clg_upstream_delta_batch(clg_engine* e, clg_delta_req* reqs, uint32_t n, const uint8_t* bytes, uint32_t in_kind) {
  ENGINE_GUARD_KEEP(e);
  clg_engine::HostTimer ht(e, "host_abi_upstream");  // (CLONOS_HOST_PROF: lock held to here; settle and the call)
  e->settle();
  if (n && (!reqs || !bytes)) return fail(CLG_E_INVALID_ARG, "null argument");
  return e->upstream_batch(reqs, n, bytes, in_kind);
}

int clg_consumer_seek_batch(clg_engine* e, const clg_slice_req* reqs, const int32_t* offsets, uint32_t n) {
  ENGINE_GUARD_KEEP(e);
  if (n && (!reqs || !offsets)) return fail(CLG_E_INVALID_ARG, "null argument");
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(e->get_log(reqs[i].log, &l));
    auto it = l->epochs.find(reqs[i].epoch);
    if (it == l->epochs.end()) return fail(CLG_E_STATE, "epoch %lld not in log", (long long)reqs[i].epoch);
    l->consumers[ChKey{reqs[i].consumer.lo, reqs[i].consumer.hi}] = Consumer{EpochMap::ref(*it), offsets[i]};
  }
  return CLG_OK;
}

int clg_truncate_all(clg_engine* e, uint32_t job, int64_t cp, int32_t* applied) {  // JobCausalLogImpl :230-246
  // Beside queued asynchronous decodes whose ranges start at or above cp (config 4's step:
  // the host truncates while the GPU decodes the new epoch): the truncation only drops bytes
  // below cp, so the queued kernels read nothing it frees -- its segments return to the pool
  // once those decodes complete.  Otherwise (a decode from below cp, appends not yet flushed)
  // the queued decodes complete first.
  ENGINE_GUARD_KEEP(e);
  bool defer = false;
  if (e->any_active()) {
    int64_t mn = INT64_MAX;
    for (const auto& d : e->pq)
      if (d.active) mn = std::min(mn, d.min_epoch);
    const bool dirty = !e->dirty.empty();  // (appends not yet flushed: the flush below writes segments)
    if (cp > mn || dirty) CHK(e->settle());
    else defer = true;
  } else {
    e->release_later();
  }
  if (applied) *applied = 0;
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  Job& j = e->jobs[job];
  if (j.latest_cp >= cp) return CLG_OK;  // the CAS: only a newer checkpoint fans out
  j.latest_cp = cp;
  ++e->rebase_gen;
  std::vector<uint32_t>& to = defer ? e->free_later : e->free_segs;
  CHK(e->flush());
  clg_engine::HostTimer ht(e, "host_truncate_all");
  if (e->logs.size() >= clg_engine::kParallelLogs) {
    // 66 k logs (config 4): the host threads take parts of the log table.  A log whose epochs
    // below cp hold shared EpochStart objects (a consumer refers to them) is left to this
    // thread (their blocks go back to a per-thread free list); each part collects its freed
    // segments, which join the pool after.
    WorkPool* wp = e->workers();
    const unsigned P = wp->size();
    const size_t nl = e->logs.size(), per = (nl + P - 1) / P;
    std::vector<std::vector<uint32_t>> freed(P), later(P);
    std::vector<int> st(P, CLG_OK);
    wp->run([&](unsigned k, unsigned) {
      const size_t i1 = std::min(nl, (k + 1) * per);
      for (size_t i = k * per; i < i1; ++i) {
        if (i + 8 < i1) {  // the Log objects ahead (per-log work is bound by their cache misses)
          const char* q = reinterpret_cast<const char*>(&e->logs[i + 8]);
          for (size_t b = 0; b < sizeof(Log); b += 64) __builtin_prefetch(q + b, 1);
        }
        Log& l = e->logs[i];
        if (!l.open || l.job != job) continue;
        bool shared = false;
        for (const EpochEnt& x : l.epochs) {
          if (x.id >= cp) break;
          shared |= x.shared != nullptr;
        }
        if (shared) {
          later[k].push_back(uint32_t(i));
          continue;
        }
        if ((st[k] = e->checkpoint_complete(l, cp, freed[k])) != CLG_OK) return;
      }
    });
    ht.lap("host_trunc_pool");
    for (unsigned k = 0; k < P; ++k) to.insert(to.end(), freed[k].begin(), freed[k].end());
    for (unsigned k = 0; k < P; ++k)
      if (st[k] != CLG_OK) return fail(st[k], "checkpoint completion failed on a log (state outside its bounds)");
    size_t n_later = 0;
    for (unsigned k = 0; k < P; ++k) {
      n_later += later[k].size();
      for (uint32_t i : later[k]) CHK(e->checkpoint_complete(e->logs[i], cp, to));
    }
    ht.lap(n_later ? "host_trunc_later" : "host_trunc_free");
  } else {
    for (auto& l : e->logs)
      if (l.open && l.job == job) CHK(e->checkpoint_complete(l, cp, to));
  }
  if (applied) *applied = 1;
  return CLG_OK;
}

}  // extern "C"

// ---- typed replay columns (columns.h) -------------------------------------------------------
// The stable partition of a decoded batch by determinant class, from the decode's output where
// it lies: count and scan, the host's capacity check on the scan's totals, then the write, the
// span bases and the wide rows' v0.  LogReplayerImpl (LogReplayerImpl.java:61-119) asks for one
// typed value at a time and never for a record's offset: the columns are what it consumes.
namespace {

// ---- placement (placement.h): where the kernels of this family read and write ------------------
static_assert(clg::kPlaceHost == CLG_MEM_HOST && clg::kPlaceDevice == CLG_MEM_DEVICE && clg::kPlaceMapped == CLG_MEM_MAPPED,
              "placement.h numbers the memory kinds as the ABI does");
using clg::mem_kind_ok;
using clg::PlacePolicy;
using clg::PlaceSpec;

// The placement of n arrays of one memory kind; a misaligned or (reject_unresolved) unregistered
// array fails the call, naming `what` the arrays are.
int place_arrays(const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what, clg::Placement* pl) {
  *pl = clg::place(s, n, kind, policy, clg_mapped_device_address);
  if (pl->verdict != clg::PlaceVerdict::misaligned && pl->verdict != clg::PlaceVerdict::not_registered) return CLG_OK;
  return fail(CLG_E_INVALID_ARG, "%s array %d is not %s", what, pl->bad,
              pl->verdict == clg::PlaceVerdict::misaligned ? "aligned to its element"
                                                           : "inside memory registered with clg_host_register");
}
// A copy to or from a caller's array (the source of a host-to-device copy, else the destination),
// in pieces that cross no edge of a registered range: an array need not lie wholly inside one.
int copy_caller(clg_engine* e, void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind,
                uint32_t mem_kind = CLG_MEM_HOST) {
  const char* caller = static_cast<const char*>(kind == hipMemcpyHostToDevice ? src : dst);
  for (uint64_t at = 0, k; at < bytes; at += k) {
    k = mem_kind == CLG_MEM_DEVICE ? bytes : clg_mapped_piece(caller + at, bytes - at);  // (device memory: one copy)
    HIPCHK(hipMemcpyAsync(static_cast<char*>(dst) + at, static_cast<const char*>(src) + at, k, kind, e->stream));
  }
  return CLG_OK;
}
// The placement of outputs; staged: `buf` grown to the slots, `extra` bytes behind them and 16
// spare, and the arrays bound to their slots.
int place_out(DevBuf& buf, const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what, clg::Placement* pl,
              size_t extra = 0) {
  CHK(place_arrays(s, n, kind, policy, what, pl));
  if (!pl->staged()) return CLG_OK;
  CHK(buf.ensure(pl->total + extra + 16));
  pl->bind(s, n, buf.p);
  return CLG_OK;
}
// The placement of inputs: the same, and a staged array's copy in queued (not an absent or empty one's).
int place_in(clg_engine* e, DevBuf& buf, const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what,
             clg::Placement* pl, size_t extra = 0) {
  CHK(place_out(buf, s, n, kind, policy, what, pl, extra));
  for (int i = 0; i < n && pl->staged(); ++i)
    if (s[i].p && s[i].bytes) CHK(copy_caller(e, pl->at<void>(i), s[i].p, s[i].bytes, hipMemcpyHostToDevice));
  return CLG_OK;
}
// A staged output's copies out, queued behind the kernels that filled the slots (no-op in place).
int stage_out(clg_engine* e, const PlaceSpec* s, int n, const clg::Placement& pl) {
  for (int i = 0; i < n && pl.staged(); ++i)
    if (s[i].p && s[i].bytes) CHK(copy_caller(e, const_cast<void*>(s[i].p), pl.at<void>(i), s[i].bytes, hipMemcpyDeviceToHost));
  return CLG_OK;
}

// The input's array that column array i passes through unchanged (null: the kernels compute it).
const void* col_through(const clg_decoded& in, int i) {
  const void* const src[clg::kColArrays] = {in.tag,  nullptr,      nullptr,      nullptr,  nullptr, in.w_idx, in.w_rc,
                                            in.w_v1, in.w_var_off, in.w_var_len, in.w_sub, nullptr};
  return src[i];
}
// The two failures columnize_small and columnize_device share.
int col_bad_tag(clg_columns* out, const uint64_t* span_rec_base, uint32_t n_spans, uint64_t index, uint64_t tag) {
  out->err_status = CLG_E_INVALID_ARG;
  out->err_span = clg::col_span_of(span_rec_base, n_spans, index);
  out->err_off = int64_t(index);
  out->err_tag = int32_t(tag);
  return fail(CLG_E_INVALID_ARG, "record %llu has tag %llu", (unsigned long long)index, (unsigned long long)tag);
}
int col_too_small(const char* name, uint64_t n, const uint64_t tot[clg::kColClasses]) {
  return fail(CLG_E_CAPACITY, "column %s is too small (records %llu; totals %llu %llu %llu %llu %llu)", name,
              (unsigned long long)n, (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2],
              (unsigned long long)tot[3], (unsigned long long)tot[4]);
}

// A batch of at most kColSmallRecords records and kColSmallSpans spans, in one launch
// (k_col_small): the kernel does the check below itself and reports it in pinned memory, so the
// call has one host sync (two for CLG_MEM_HOST outputs, whose packed size is known only then).
// columnize_device has checked the arguments.
int columnize_small(clg_engine* e, const clg_decoded& in, const uint64_t* span_rec_base, uint32_t n_spans,
                    clg_columns* out) {
  const uint64_t n = in.n_rec, nw = in.n_wide;
  const bool sizes_only = clg::col_sizes_only(*out);
  const bool want_sb = out->span_base && n_spans;
  // pinned: result block | span bases | span boundaries
  const size_t o_sb = clg_engine::al16(sizeof(clg::ColSmallRes)), sbn = size_t(n_spans) + 1;
  const size_t o_srb = o_sb + sbn * clg::kColClasses * 8;
  CHK(e->h_colsmall.ensure(o_srb + sbn * 8));
  uint8_t* hp = e->h_colsmall.as<uint8_t>();
  clg::ColSmallRes* res = reinterpret_cast<clg::ColSmallRes*>(hp);
  uint64_t* h_sb = reinterpret_cast<uint64_t*>(hp + o_sb);
  uint64_t* h_srb = reinterpret_cast<uint64_t*>(hp + o_srb);
  if (want_sb) memcpy(h_srb, span_rec_base, sbn * 8);

  // where the kernel writes: the caller's device arrays, the device side of registered host
  // arrays, or (plain host memory, and registered memory that is not wholly inside one registered
  // range) one packed engine buffer that is read back in one copy.  The registry is asked for
  // each array's capacity, not its length: the lengths are known only after the one launch.
  PlaceSpec spec[clg::kColArrays];
  for (int i = 0; i < clg::kColArrays; ++i)
    spec[i] = {clg::col_ptr(*out, i), clg::col_array_cap(*out, i) * clg::kColArray[i].width, clg::kColArray[i].width};
  clg::Placement pl;
  CHK(place_arrays(spec, clg::kColArrays, out->out_kind, PlacePolicy::stage_if_unresolved, "column", &pl));
  const bool packed = pl.staged();
  void* dev[clg::kColArrays];
  for (int i = 0; i < clg::kColArrays; ++i) dev[i] = pl.at<void>(i);
  clg::ColSmallOut so{};
  if (packed && !sizes_only) {
    CHK(e->d_colout.ensure(clg::col_pack_bound(n, nw) + 16));
    so.pack = e->d_colout.as<uint8_t>();
  } else if (!sizes_only) {
    for (int i = 0; i < clg::kColArrays; ++i)  // (an array that is the input's own stays as it is)
      if (dev[i] == col_through(in, i)) dev[i] = nullptr;
    so.tag = static_cast<uint8_t*>(dev[0]), so.order = static_cast<int8_t*>(dev[1]);
    so.timestamp = static_cast<int64_t*>(dev[2]), so.rng = static_cast<int32_t*>(dev[3]);
    so.buffer_built = static_cast<int32_t*>(dev[4]), so.w_idx = static_cast<uint32_t*>(dev[5]);
    so.w_rc = static_cast<int32_t*>(dev[6]), so.w_v1 = static_cast<int64_t*>(dev[7]);
    so.w_var_off = static_cast<uint32_t*>(dev[8]), so.w_var_len = static_cast<uint32_t*>(dev[9]);
    so.w_sub = static_cast<uint8_t*>(dev[10]), so.w_v0 = static_cast<int64_t*>(dev[11]);
  }
  for (int i = 0; i < clg::kColNarrowArrays; ++i) so.cap[i] = clg::col_array_cap(*out, i);
  so.cap[5] = out->cap_wide;  // (the wide arrays share one capacity: none when one of them is absent)
  for (int i = clg::kColNarrowArrays; i < clg::kColArrays; ++i) so.cap[5] = std::min(so.cap[5], clg::col_array_cap(*out, i));
  const clg::ColSmallIn si{in.tag,       in.v0,       in.w_idx, in.w_rc, in.w_v1, in.w_var_off,
                           in.w_var_len, in.w_sub,    want_sb ? h_srb : nullptr,  n,       nw,
                           want_sb ? n_spans : 0u, sizes_only ? 1u : 0u};
  e->stats["columns_small"].launches++;
  // (bytes: the tags twice and v0 once, the columns, the side rows in and out; as the multi-kernel form counts them)
  const uint64_t moved = (want_sb ? sbn * 48 : 0) + (sizes_only ? n : 2 * n + 8 * n + 8 * (n - std::min(n, nw)) + 58 * nw);
  CHK(e->timed("decode_columns", moved, [&] { return clg::launch_col_small(si, so, res, want_sb ? h_sb : nullptr, e->stream); }));
  CHK(e->sync());
  out->n_rec = n;
  if (res->verdict == clg::kColSmallBadTag) return col_bad_tag(out, span_rec_base, n_spans, res->bad_index, res->bad_tag);
  uint64_t tot[clg::kColClasses];
  for (uint32_t c = 0; c < clg::kColClasses; ++c) out->n_class[c] = tot[c] = res->total[c];
  if (res->verdict == clg::kColSmallWideCount)
    return fail(CLG_E_INVALID_ARG, "n_wide is %llu, the tags hold %llu wide records", (unsigned long long)nw,
                (unsigned long long)tot[clg::kColWide]);
  if (res->verdict == clg::kColSmallWritten && packed && res->pack_off[12]) {
    const uint64_t end = res->pack_off[12];
    if (end > clg::col_pack_bound(n, nw)) return fail(CLG_E_DEVICE, "the packed columns end at %llu", (unsigned long long)end);
    CHK(e->h_colpack.ensure(end));
    HIPCHK(hipMemcpyAsync(e->h_colpack.p, so.pack, end, hipMemcpyDeviceToHost, e->stream));
    CHK(e->sync());
    for (int i = 0; i < clg::kColArrays; ++i)
      if (const uint64_t cnt = clg::col_array_len(i, n, tot))
        memcpy(clg::col_ptr(*out, i), e->h_colpack.as<uint8_t>() + res->pack_off[i], cnt * clg::kColArray[i].width);
  }
  if (out->span_base) {
    if (n_spans) memcpy(out->span_base, h_sb, sbn * 8 * clg::kColClasses);
    else memcpy(out->span_base, tot, sizeof tot);
  }
  // (short_cap: the narrow array's index, 5 for the wide arrays)
  if (res->verdict == clg::kColSmallCapacity) return col_too_small(clg::kColArray[std::min(res->short_cap, 5u)].name, n, tot);
  return CLG_OK;
}

// `in`: device addresses (the caller's device arrays, engine scratch, or the device side of
// registered host memory).
int columnize_device(clg_engine* e, const clg_decoded& in, const uint64_t* span_rec_base, uint32_t n_spans,
                     clg_columns* out) {
  clg::col_reset_result(out);
  const uint64_t n = in.n_rec, nw = in.n_wide;
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  if ((n && (!in.tag || !in.v0)) || (nw && (!in.w_idx || !in.w_rc || !in.w_v1 || !in.w_var_off || !in.w_var_len || !in.w_sub)))
    return fail(CLG_E_INVALID_ARG, "null input array");
  if (!clg::col_spans_ok(span_rec_base, n_spans, n))
    return fail(CLG_E_INVALID_ARG, "span_rec_base decreases or passes n_rec");
  if ((n + clg::kColTile - 1) / clg::kColTile >> 31) return fail(CLG_E_INVALID_ARG, "%llu records in one call", (unsigned long long)n);
  for (int i = 0; i < clg::kColArrays && out->out_kind != CLG_MEM_HOST; ++i)  // (an empty array's too: no length is known yet)
    if (uintptr_t(clg::col_ptr(*out, i)) % clg::kColArray[i].width)
      return fail(CLG_E_INVALID_ARG, "column %d is not aligned to its element", i);
  if (e->sw.columns_small && n <= clg::kColSmallRecords && n_spans <= clg::kColSmallSpans)
    return columnize_small(e, in, span_rec_base, n_spans, out);
  const uint32_t n_tiles = uint32_t((n + clg::kColTile - 1) / clg::kColTile);
  const clg::ColIn cin{in.tag, in.v0, in.w_idx, n, nw};

  // count and scan; the totals come back before anything is written to the caller
  CHK(e->d_colcnt.ensure(size_t(n_tiles) * clg::kColCountWords * 4 + 64));
  CHK(e->d_colbase.ensure(size_t(n_tiles) * clg::kColClasses * 8 + 64));
  CHK(e->h_colres.ensure(sizeof(clg::ColRes)));
  clg::ColRes* res = e->h_colres.as<clg::ColRes>();
  CHK(e->timed("decode_columns", n, [&] {
    return clg::launch_col_count_scan(cin, n_tiles, e->d_colcnt.as<uint32_t>(), e->d_colbase.as<uint64_t>(), res, e->stream);
  }));
  CHK(e->sync());
  out->n_rec = n;
  if (res->bad_tile != clg::kColNoTile) {  // a tag above 7: one wave finds the record
    CHK(clg::launch_col_find_bad(cin, res->bad_tile, res, e->stream));
    CHK(e->sync());
    return col_bad_tag(out, span_rec_base, n_spans, res->bad_index, res->bad_tag);
  }
  uint64_t tot[clg::kColClasses];
  for (uint32_t c = 0; c < clg::kColClasses; ++c) out->n_class[c] = tot[c] = res->total[c];
  if (tot[clg::kColWide] != nw)
    return fail(CLG_E_INVALID_ARG, "n_wide is %llu, the tags hold %llu wide records", (unsigned long long)nw,
                (unsigned long long)tot[clg::kColWide]);
  const bool sizes_only = clg::col_sizes_only(*out);
  const char* short_col = sizes_only ? nullptr : clg::col_short_column(*out, n, tot);
  const bool write = !sizes_only && !short_col;

  // where the kernels write: the caller's device arrays, the device side of registered host
  // arrays, or engine staging (plain host memory, and registered memory that is not wholly
  // inside one registered range).  Only the arrays the kernels write, each with its length (known
  // here, unlike in columnize_small); those passed through are copied below and absent here.
  PlaceSpec wr[clg::kColArrays];
  for (int i = 0; i < clg::kColArrays; ++i)
    wr[i] = {col_through(in, i) ? nullptr : clg::col_ptr(*out, i), clg::col_array_len(i, n, tot) * clg::kColArray[i].width,
             clg::kColArray[i].width};
  clg::Placement pl;
  if (write) CHK(place_out(e->d_colout, wr, clg::kColArrays, out->out_kind, PlacePolicy::stage_if_unresolved, "column", &pl));
  const clg::ColOut cout_{pl.at<int8_t>(1), pl.at<int64_t>(2), pl.at<int32_t>(3), pl.at<int32_t>(4), pl.at<int64_t>(11)};
  const bool want_sb = out->span_base && n_spans;
  if (want_sb) {
    const size_t sb = size_t(n_spans + 1) * 8;
    CHK(e->h_colsb.ensure(sb * clg::kColClasses));
    CHK(e->d_colsrb.ensure(sb));
    CHK(e->d_colsb.ensure(sb * clg::kColClasses));
    memcpy(e->h_colsb.p, span_rec_base, sb);
    HIPCHK(hipMemcpyAsync(e->d_colsrb.p, e->h_colsb.p, sb, hipMemcpyHostToDevice, e->stream));
  }
  uint64_t moved = n_tiles * uint64_t(clg::kColClasses) * 8 + (want_sb ? uint64_t(n_spans + 1) * 48 : 0);
  if (write) moved += n + 8 * (n - nw) + tot[0] + 8 * tot[1] + 4 * tot[2] + 4 * tot[3] + 20 * nw;
  CHK(e->timed("decode_columns", moved, [&] {
    return clg::launch_col_write(cin, n_tiles, e->d_colbase.as<uint64_t>(), res, write, cout_,
                                 want_sb ? e->d_colsrb.as<uint64_t>() : nullptr, n_spans, e->d_colsb.as<uint64_t>(), e->stream);
  }));
  if (want_sb)  // (h_colsb's copy of span_rec_base was uploaded by the copy queued before the kernels)
    HIPCHK(hipMemcpyAsync(e->h_colsb.p, e->d_colsb.p, size_t(n_spans + 1) * 8 * clg::kColClasses, hipMemcpyDeviceToHost, e->stream));
  if (write) {
    // the arrays that stay as they are: the tags and the side rows
    for (int i = 0; i < clg::kColArrays; ++i) {
      const void* src = col_through(in, i);
      void* dst = clg::col_ptr(*out, i);
      if (src && wr[i].bytes && dst != src) CHK(copy_caller(e, dst, src, wr[i].bytes, hipMemcpyDefault, out->out_kind));
    }
    CHK(stage_out(e, wr, clg::kColArrays, pl));
  }
  CHK(e->sync());
  if (out->span_base) {
    if (n_spans) memcpy(out->span_base, e->h_colsb.p, size_t(n_spans + 1) * 8 * clg::kColClasses);
    else memcpy(out->span_base, tot, sizeof tot);
  }
  if (short_col) return col_too_small(short_col, n, tot);
  return CLG_OK;
}

// The decode into engine scratch (the host-output staging arrays, kept between calls), grown
// and run again on the decode's own CLG_E_CAPACITY, then the columns of what it produced.
// keep (optional): the decoded batch in engine scratch and columnize_device's own status, for
// the payload column of the same rows (decode_columns_var).
struct ColKeep {
  clg_decoded d{};
  bool valid = false;        // the decode produced a batch and columnize_device ran
  int col_status = CLG_OK;   // columnize_device's
};
int decode_columns(clg_engine* e, const std::function<int(clg_decoded*, uint64_t*)>& run, uint32_t n_spans,
                   clg_columns* out, ColKeep* keep = nullptr) {
  clg::col_reset_result(out);
  std::vector<uint64_t> base(size_t(n_spans) + 1, 0);
  clg_decoded d{};
  uint64_t need = 1u << 16, wneed = 1u << 12;
  int st = CLG_OK;
  for (int round = 0;; ++round) {
    CHK(e->d_o_off.ensure(need * 4));
    CHK(e->d_o_tag.ensure(need));
    CHK(e->d_o_v0.ensure(need * 8));
    CHK(e->d_o_widx.ensure(wneed * 4));
    CHK(e->d_o_wrc.ensure(wneed * 4));
    CHK(e->d_o_wv1.ensure(wneed * 8));
    CHK(e->d_o_wvo.ensure(wneed * 4));
    CHK(e->d_o_wvl.ensure(wneed * 4));
    CHK(e->d_o_wsub.ensure(wneed));
    d = clg_decoded{};
    d.off = e->d_o_off.as<uint32_t>(), d.tag = e->d_o_tag.as<uint8_t>(), d.v0 = e->d_o_v0.as<int64_t>();
    d.w_idx = e->d_o_widx.as<uint32_t>(), d.w_rc = e->d_o_wrc.as<int32_t>(), d.w_v1 = e->d_o_wv1.as<int64_t>();
    d.w_var_off = e->d_o_wvo.as<uint32_t>(), d.w_var_len = e->d_o_wvl.as<uint32_t>(), d.w_sub = e->d_o_wsub.as<uint8_t>();
    d.cap = std::min({uint64_t(e->d_o_off.cap / 4), uint64_t(e->d_o_tag.cap), uint64_t(e->d_o_v0.cap / 8)});
    d.wcap = std::min({uint64_t(e->d_o_widx.cap / 4), uint64_t(e->d_o_wrc.cap / 4), uint64_t(e->d_o_wv1.cap / 8),
                       uint64_t(e->d_o_wvo.cap / 4), uint64_t(e->d_o_wvl.cap / 4), uint64_t(e->d_o_wsub.cap)});
    d.out_kind = CLG_MEM_DEVICE;
    st = run(&d, base.data());
    if (st != CLG_E_CAPACITY || round == 2) break;
    need = std::max<uint64_t>(d.n_rec, d.cap);  // (the decode reported what it produced)
    wneed = std::max<uint64_t>(d.n_wide, d.wcap);
  }
  if (st == CLG_E_CAPACITY) return st;
  if (st != CLG_OK && d.err_status == CLG_OK) return st;  // an engine failure, not a decode result
  const std::string decode_err = st != CLG_OK ? g_err : std::string();
  const int col_status = columnize_device(e, d, base.data(), n_spans, out);
  if (keep) keep->d = d, keep->valid = true, keep->col_status = col_status;
  CHK(col_status);
  out->err_status = d.err_status;
  out->err_span = d.err_span;
  out->err_off = d.err_off;
  out->err_tag = d.err_tag;
  if (st != CLG_OK) g_err = decode_err;
  return st;
}

// ---- the payload column (payload.h) ---------------------------------------------------------
// The wide rows' payload bytes packed in row order: size and scan, the host's check of the
// scan's totals, then pos and the copy.  Host work is O(spans + segments covered): a PaySpan per
// span and the segment table; the rows stay on the device.
//
// At most kPaySmallRows rows over spans of at most kPaySmallBytes bytes, in one launch
// (k_pay_small): the kernel does the check itself and reports it in pinned memory.  One host sync
// (two for outputs that are not device memory: pos | var come back packed in one copy).
// gather_payloads_device has checked the arguments and uploaded the descriptors behind `in`.
int gather_payloads_small(clg_engine* e, const clg::PayIn& in, clg_payloads* out, bool sizes_only, uint64_t span_bytes,
                          uint64_t desc_bytes) {
  const uint64_t n = in.n_rows;
  CHK(e->h_payres.ensure(sizeof(clg::PaySmallRes)));
  clg::PaySmallRes* res = e->h_payres.as<clg::PaySmallRes>();
  const uint64_t cap_pos = out->pos ? out->cap_pos : 0, cap_var = out->var ? out->cap_var : 0;
  // where the kernel writes: the caller's device arrays, or (host and registered memory alike:
  // the short rows' byte stores stay off the link) engine staging, pos | var; sizes only: nowhere.
  // Staging holds what the spans hold.  Rows of a caller may overlap, so n_var can be more: then
  // the kernel reports the staging as short, and runs once more with staging of n_var bytes.
  PlaceSpec dst[2] = {{out->pos, (n + 1) * 8, 8}, {out->var, std::min(cap_var, span_bytes), 1}};
  clg::Placement pl;
  e->stats["payloads_small"].launches++;
  for (int round = 0;; ++round) {
    if (!sizes_only) CHK(place_out(e->d_payout, dst, 2, out->out_kind, PlacePolicy::stage_unless_device, "payload", &pl));
    CHK(e->timed("decode_payloads", n * 20 + (n + 1) * 8 + desc_bytes, [&] {
      return clg::launch_pay_small(in, pl.at<uint64_t>(0), pl.at<uint8_t>(1), cap_pos, pl.staged() ? dst[1].bytes : cap_var,
                                   sizes_only, res, e->stream);
    }));
    CHK(e->sync());
    if (round || !pl.staged() || res->verdict != clg::kPaySmallCapacity || !res->short_cap || res->n_var > cap_var) break;
    dst[1].bytes = res->n_var;
  }
  out->n_var = res->n_var;
  if (res->verdict == clg::kPaySmallBadRow) {
    out->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "row %llu passes its span's end", (unsigned long long)res->bad_row);
  }
  if (res->verdict == clg::kPaySmallCapacity)
    return fail(CLG_E_CAPACITY, "%s is too small (rows %llu, payload bytes %llu)", res->short_cap ? "var" : "pos",
                (unsigned long long)n, (unsigned long long)res->n_var);
  if (res->verdict == clg::kPaySmallWritten && pl.staged()) {  // pos | var come back in one copy
    const uint64_t nv = res->n_var, pb = pl.off[1];
    CHK(e->h_paypack.ensure(pb + nv));
    HIPCHK(hipMemcpyAsync(e->h_paypack.p, pl.at<void>(0), pb + nv, hipMemcpyDeviceToHost, e->stream));
    CHK(e->sync());
    memcpy(out->pos, e->h_paypack.p, (n + 1) * 8);
    if (nv) memcpy(out->var, e->h_paypack.as<uint8_t>() + pb, nv);
  }
  return CLG_OK;
}

// d_off / d_len: device addresses of the rows.  sizes_forced: fill the results, write nothing.
int gather_payloads_device(clg_engine* e, const std::vector<clg::PaySpan>& spans, const std::vector<uint32_t>& segtab,
                           const uint32_t* d_off, const uint32_t* d_len, const uint64_t* row_base, clg_payloads* out,
                           bool sizes_forced = false) {
  const uint32_t ns = uint32_t(spans.size());
  clg::pay_reset_result(out);
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  if (!clg::pay_row_base_ok(row_base, ns)) return fail(CLG_E_INVALID_ARG, "row_base does not start at 0 or decreases");
  const uint64_t n = ns ? row_base[ns] : 0;
  if (n > 0xFFFFFFFFull) return fail(CLG_E_INVALID_ARG, "%llu rows in one call", (unsigned long long)n);
  out->n_rows = n;
  const bool sizes_only = sizes_forced || clg::pay_sizes_only(*out);
  const bool direct = out->out_kind == CLG_MEM_DEVICE;
  if (!sizes_only && direct && uintptr_t(out->pos) % 8) return fail(CLG_E_INVALID_ARG, "pos is not aligned to its element");
  if (!n) {  // no rows: only pos[0]
    if (sizes_only) return CLG_OK;
    if (const char* name = clg::pay_short(*out, 0, 0)) return fail(CLG_E_CAPACITY, "%s is too small (rows 0)", name);
    const uint64_t zero = 0;
    if (direct) HIPCHK(hipMemcpy(out->pos, &zero, 8, hipMemcpyHostToDevice));
    else out->pos[0] = 0;
    return CLG_OK;
  }
  if (!d_off || !d_len) return fail(CLG_E_INVALID_ARG, "null row array");
  const uint32_t n_tiles = uint32_t((n + clg::kPayTile - 1) / clg::kPayTile);

  // span table | row_base | segment table, in one upload
  const size_t sb = size_t(ns) * sizeof(clg::PaySpan), rb = size_t(ns + 1) * 8, tb = segtab.size() * 4;
  CHK(e->h_paydesc.ensure(sb + rb + tb + 16));
  CHK(e->d_paydesc.ensure(sb + rb + tb + 16));
  uint8_t* h = e->h_paydesc.as<uint8_t>();
  memcpy(h, spans.data(), sb);
  memcpy(h + sb, row_base, rb);
  if (tb) memcpy(h + sb + rb, segtab.data(), tb);
  HIPCHK(hipMemcpyAsync(e->d_paydesc.p, h, sb + rb + tb, hipMemcpyHostToDevice, e->stream));
  const uint8_t* dd = e->d_paydesc.as<uint8_t>();
  const clg::PayIn in{d_off, d_len, reinterpret_cast<const uint64_t*>(dd + sb), reinterpret_cast<const clg::PaySpan*>(dd),
                      reinterpret_cast<const uint32_t*>(dd + sb + rb), e->pool, n, ns, e->C()};
  uint64_t span_bytes = 0;  // (an upper bound of n_var)
  for (const clg::PaySpan& sp : spans) span_bytes += sp.len;
  if (e->sw.columns_small && n <= clg::kPaySmallRows && span_bytes <= clg::kPaySmallBytes)
    return gather_payloads_small(e, in, out, sizes_only, span_bytes, sb + rb);
  CHK(e->d_paytile.ensure(size_t(n_tiles) * 24 + 64));
  uint64_t* d_sum = e->d_paytile.as<uint64_t>();
  uint64_t* d_bad = d_sum + n_tiles;
  uint64_t* d_base = d_bad + n_tiles;
  CHK(e->h_payres.ensure(sizeof(clg::PayRes)));
  clg::PayRes* res = e->h_payres.as<clg::PayRes>();

  // size and scan; the totals come back before anything is written to the caller
  CHK(e->timed("decode_payloads", n * 8 + uint64_t(n_tiles) * 40 + sb + rb, [&] {
    return clg::launch_pay_size_scan(in, n_tiles, d_sum, d_bad, d_base, res, e->stream);
  }));
  CHK(e->sync());
  out->n_var = res->n_var;
  if (res->bad_row != clg::kPayNoRow) {
    out->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "row %llu passes its span's end", (unsigned long long)res->bad_row);
  }
  if (sizes_only) return CLG_OK;
  const uint64_t nv = res->n_var;
  if (const char* name = clg::pay_short(*out, n, nv))
    return fail(CLG_E_CAPACITY, "%s is too small (rows %llu, payload bytes %llu)", name, (unsigned long long)n,
                (unsigned long long)nv);

  // where the kernels write: the caller's device arrays, or engine staging and one copy each
  // (host and registered memory alike: the short rows' byte stores stay off the link)
  const PlaceSpec dst[2] = {{out->pos, (n + 1) * 8, 8}, {out->var, nv, 1}};
  clg::Placement pl;
  CHK(place_out(e->d_payout, dst, 2, out->out_kind, PlacePolicy::stage_unless_device, "payload", &pl));
  CHK(e->timed("decode_payloads", n * 12 + (n + 1) * 8 + uint64_t(n_tiles) * 8 + 2 * nv, [&] {
    return clg::launch_pay_write(in, n_tiles, d_base, nv, pl.at<uint64_t>(0), pl.at<uint8_t>(1), e->stream);
  }));
  CHK(stage_out(e, dst, 2, pl));
  return e->sync();
}

// The rows of a caller: device arrays as they are, host arrays staged.
int stage_payload_rows(clg_engine* e, const uint32_t* off, const uint32_t* len, uint64_t n, uint32_t in_kind,
                       const uint32_t** d_off, const uint32_t** d_len) {
  *d_off = off;
  *d_len = len;
  if (in_kind != CLG_MEM_HOST || !n) return CLG_OK;
  if (!off || !len) return fail(CLG_E_INVALID_ARG, "null row array");
  const PlaceSpec rows[2] = {{off, n * 4, 4}, {len, n * 4, 4}};
  clg::Placement pl;
  CHK(place_in(e, e->d_payrows, rows, 2, in_kind, PlacePolicy::stage_unless_device, "row", &pl));
  *d_off = pl.at<const uint32_t>(0);
  *d_len = pl.at<const uint32_t>(1);
  return CLG_OK;
}

// Spans of one buffer (host input staged as clg_decode_host stages it) as contiguous PaySpans.
int payload_spans_bytes(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                        uint32_t n, uint32_t in_kind, std::vector<clg::PaySpan>& spans) {
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) total += span_len[i];
  if (total && !bytes) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint8_t* base = bytes;
  uint64_t base_off = 0;
  if (total) CHK(e->stage_spans(bytes, span_off, span_len, n, in_kind, &base, &base_off));
  spans.resize(n);
  for (uint32_t i = 0; i < n; ++i)
    spans[i] = clg::PaySpan{span_len[i] ? base + (span_off[i] - base_off) : nullptr, 0, span_len[i], 0, 0};
  return CLG_OK;
}

// getDeterminants(start_epoch[i]) of log[i], in place: plan_log_span's run and table entries.
int payload_spans_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                       std::vector<clg::PaySpan>& spans, std::vector<uint32_t>& segtab) {
  CHK(e->flush());
  spans.resize(n);
  const uint32_t C = e->C();
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(e->get_log(log[i], &l));
    int32_t s = 0, nb = 0;
    if (l->depth != 0) CHK(e->determinants_range(*l, start_epoch[i], &s, &nb));
    spans[i] = clg::PaySpan{nullptr, segtab.size(), uint64_t(nb), 0, 0};
    if (nb > 0) {  // only the segments the span covers go into the table (phys rebased on them)
      const uint32_t s0 = uint32_t(s) / C, s1 = uint32_t(s + nb - 1) / C + 1;
      spans[i].phys = uint32_t(s) - s0 * C;
      segtab.insert(segtab.end(), l->segs.begin() + s0, l->segs.begin() + s1);
    }
  }
  return CLG_OK;
}

// decode_columns, then the payloads of the wide rows it produced (row_base: the columns' wide
// span bases).  The columns' status wins when it is not CLG_OK.
int decode_columns_var(clg_engine* e, const std::function<int(clg_decoded*, uint64_t*)>& run, uint32_t n,
                       clg_columns* out, clg_payloads* var,
                       const std::function<int(std::vector<clg::PaySpan>&, std::vector<uint32_t>&)>& spans_of) {
  clg::pay_reset_result(var);
  std::vector<uint64_t> own_sb;
  uint64_t* const caller_sb = out->span_base;
  if (!caller_sb) {  // (the wide bases are needed whether or not the caller asked for them)
    own_sb.assign(size_t(n + 1) * clg::kColClasses, 0);
    out->span_base = own_sb.data();
  }
  ColKeep keep;
  const int cs = decode_columns(e, run, n, out, &keep);
  const std::string col_err = g_err;
  std::vector<uint64_t> row_base(size_t(n) + 1);
  for (uint32_t s = 0; s <= n; ++s) row_base[s] = out->span_base[size_t(s) * clg::kColClasses + clg::kColWide];
  out->span_base = caller_sb;
  if (!keep.valid || (keep.col_status != CLG_OK && keep.col_status != CLG_E_CAPACITY)) return cs;
  std::vector<clg::PaySpan> spans;
  std::vector<uint32_t> segtab;
  int ps = spans_of(spans, segtab);
  if (ps == CLG_OK)
    ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var,
                                keep.col_status == CLG_E_CAPACITY);
  if (cs != CLG_OK) {
    g_err = col_err;
    return cs;
  }
  return ps;
}

// ---- packed typed columns (pack.h) ----------------------------------------------------------
// The five narrow columns bit-packed where they lie: measure and the offset scan, the host's
// capacity check on the scan's total, then the write.  A LogReplayerImpl cursor
// (LogReplayerImpl.java:61-119) pops one typed value at a time from the blocks.

// Measure and scan over device-side streams: out's results are filled, the descriptors (with
// their offsets) are left in d_packdesc.
int pack_sizes(clg_engine* e, const clg::PackSrc& src, clg_packed* out, clg::PackIn* pin) {
  clg::pack_reset_result(out);
  clg::pack_layout(src.n, out);
  const uint64_t nb = out->blk_base[clg::kPackStreams];
  if (nb >> 31) return fail(CLG_E_INVALID_ARG, "%llu blocks in one call", (unsigned long long)nb);
  uint64_t in_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) {
    if (src.n[c] && !src.col[c]) return fail(CLG_E_INVALID_ARG, "null input array (stream %u)", c);
    if (uintptr_t(src.col[c]) % clg::pack_elem(c)) return fail(CLG_E_INVALID_ARG, "stream %u is not aligned to its element", c);
    pin->col[c] = src.col[c], pin->n[c] = src.n[c];
    in_bytes += src.n[c] * clg::pack_elem(c);
  }
  for (uint32_t c = 0; c <= clg::kPackStreams; ++c) pin->blk_base[c] = out->blk_base[c];
  const uint64_t ng = (nb + clg::kPackScanGroup - 1) / clg::kPackScanGroup;
  CHK(e->d_packdesc.ensure(size_t(nb) * sizeof(clg_pack_block) + 64));
  CHK(e->d_packsum.ensure(size_t(ng) * 8 + 64));
  CHK(e->h_packres.ensure(sizeof(clg::PackRes)));
  clg::PackRes* res = e->h_packres.as<clg::PackRes>();
  // (bytes: the columns once, a descriptor written, read and written again, the groups' sums)
  CHK(e->timed("pack_columns", in_bytes + nb * 72 + ng * 24, [&] {
    return clg::launch_pack_measure_scan(*pin, uint32_t(nb), e->d_packdesc.as<clg_pack_block>(), e->d_packsum.as<uint64_t>(),
                                         res, e->stream);
  }));
  CHK(e->sync());
  out->n_bits = res->n_bits;
  return CLG_OK;
}

int pack_out_check(const clg_packed& out, const char* what = "") {  // (a packed input's, too)
  if (!mem_kind_ok(out.out_kind)) return fail(CLG_E_INVALID_ARG, "%sout_kind %u", what, out.out_kind);
  if (out.out_kind != CLG_MEM_HOST && (uintptr_t(out.desc) % 8 || uintptr_t(out.bits) % 16))
    return fail(CLG_E_INVALID_ARG, "desc must be aligned to 8 bytes and bits to 16");
  return CLG_OK;
}

// The write pass, after pack_sizes and the capacity check: device and registered outputs are
// written by the kernel, host ones through engine staging and one copy each.
int pack_write(clg_engine* e, const clg::PackIn& pin, clg_packed* out) {
  const uint64_t nb = out->blk_base[clg::kPackStreams], nbits = out->n_bits;
  if (!nb) return CLG_OK;
  const PlaceSpec dst[2] = {{out->desc, nb * sizeof(clg_pack_block), 8}, {out->bits, nbits, 16}};
  clg::Placement pl;
  CHK(place_out(e->d_packout, dst, 2, out->out_kind, PlacePolicy::stage_if_unresolved, "packed", &pl));
  uint64_t in_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) in_bytes += pin.n[c] * clg::pack_elem(c);
  CHK(e->timed("pack_columns", in_bytes + nb * 64 + nbits, [&] {
    return clg::launch_pack_write(pin, uint32_t(nb), e->d_packdesc.as<clg_pack_block>(), pl.at<clg_pack_block>(0),
                                  pl.at<uint8_t>(1), nb, nbits, e->stream);
  }));
  CHK(stage_out(e, dst, 2, pl));
  return e->sync();
}

int pack_capacity_error(const clg_packed& out, const char* name) {
  return fail(CLG_E_CAPACITY, "packed columns: %s is too small (blocks %llu, payload bytes %llu)", name,
              (unsigned long long)out.blk_base[clg::kPackStreams], (unsigned long long)out.n_bits);
}

// The decode into engine scratch and the columns of what it produced, also in engine scratch;
// then the pack, the wide rows as they are and (var) the payload column of the same rows.
// Every size is known before anything is written to the caller.
int decode_columns_packed(clg_engine* e, const std::function<int(clg_decoded*, uint64_t*)>& run, uint32_t n,
                          clg_columns* wide, clg_payloads* var, clg_packed* out,
                          const std::function<int(std::vector<clg::PaySpan>&, std::vector<uint32_t>&)>& spans_of) {
  if (wide->tag || wide->order || wide->timestamp || wide->rng || wide->buffer_built)
    return fail(CLG_E_INVALID_ARG, "the narrow column pointers of `wide` must be NULL: those columns are delivered packed");
  if (!mem_kind_ok(wide->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", wide->out_kind);
  CHK(pack_out_check(*out));
  clg::col_reset_result(wide);
  clg::pack_reset_result(out);
  if (var) clg::pay_reset_result(var);

  // the decode, and the columns' sizes and span bases
  std::vector<uint64_t> sb(size_t(n + 1) * clg::kColClasses, 0);
  clg_columns sizes{};
  sizes.span_base = sb.data();
  sizes.out_kind = CLG_MEM_DEVICE;
  ColKeep keep;
  const int cs = decode_columns(e, run, n, &sizes, &keep);
  const std::string col_err = g_err;
  wide->n_rec = sizes.n_rec;
  for (uint32_t c = 0; c < clg::kColClasses; ++c) wide->n_class[c] = sizes.n_class[c];
  wide->err_status = sizes.err_status, wide->err_span = sizes.err_span;
  wide->err_off = sizes.err_off, wide->err_tag = sizes.err_tag;
  if (!keep.valid || keep.col_status != CLG_OK) return cs;
  if (wide->span_base) memcpy(wide->span_base, sb.data(), sb.size() * 8);
  const uint64_t nr = sizes.n_rec, nw = sizes.n_class[clg::kColWide];
  const uint64_t* tot = sizes.n_class;

  // the narrow columns and w_v0 into engine scratch (the tags and the side rows stay where the
  // decode left them)
  const uint64_t cb[5] = {tot[0], tot[1] * 8, tot[2] * 4, tot[3] * 4, nw * 8};
  size_t at[6];
  CHK(e->d_packcol.ensure(clg::place_layout(cb, 5, at) + 16));
  uint8_t* sc = e->d_packcol.as<uint8_t>();
  clg_columns full{};
  full.tag = keep.d.tag, full.order = reinterpret_cast<int8_t*>(sc + at[0]);
  full.timestamp = reinterpret_cast<int64_t*>(sc + at[1]), full.rng = reinterpret_cast<int32_t*>(sc + at[2]);
  full.buffer_built = reinterpret_cast<int32_t*>(sc + at[3]), full.w_v0 = reinterpret_cast<int64_t*>(sc + at[4]);
  full.w_idx = keep.d.w_idx, full.w_rc = keep.d.w_rc, full.w_v1 = keep.d.w_v1, full.w_var_off = keep.d.w_var_off;
  full.w_var_len = keep.d.w_var_len, full.w_sub = keep.d.w_sub;
  full.cap_tag = nr, full.cap_order = tot[0], full.cap_timestamp = tot[1], full.cap_rng = tot[2];
  full.cap_buffer_built = tot[3], full.cap_wide = nw;
  full.out_kind = CLG_MEM_DEVICE;
  CHK(columnize_device(e, keep.d, nullptr, 0, &full));

  // every size, before anything is written to the caller
  const clg::PackSrc src{{full.tag, full.order, full.timestamp, full.rng, full.buffer_built}, {nr, tot[0], tot[1], tot[2], tot[3]}};
  clg::PackIn pin{};
  CHK(pack_sizes(e, src, out, &pin));
  int ps = CLG_OK;
  std::vector<clg::PaySpan> spans;
  std::vector<uint32_t> segtab;
  std::vector<uint64_t> row_base(size_t(n) + 1);
  for (uint32_t s = 0; s <= n; ++s) row_base[s] = sb[size_t(s) * clg::kColClasses + clg::kColWide];
  if (var) {
    ps = spans_of(spans, segtab);
    if (ps == CLG_OK) ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var, true);
  }
  const std::string pay_err = g_err;
  const int w0 = clg::kColNarrowArrays, w1 = clg::kColArrays;  // (the wide arrays: the table's last seven)
  bool wide_any = false, wide_short = false;
  for (int i = w0; i < w1; ++i) wide_any = wide_any || clg::col_ptr(*wide, i);
  for (int i = w0; i < w1; ++i) wide_short = wide_short || (wide_any && clg::col_array_cap(*wide, i) < nw);
  const char* pk_short = clg::pack_sizes_only(*out) ? nullptr : clg::pack_short(*out);
  const char* pay_short = var && ps == CLG_OK && !clg::pay_sizes_only(*var) ? clg::pay_short(*var, var->n_rows, var->n_var) : nullptr;
  if (wide_short) return fail(CLG_E_CAPACITY, "the wide rows' arrays are too small (rows %llu)", (unsigned long long)nw);
  if (pk_short) return pack_capacity_error(*out, pk_short);
  if (pay_short)
    return fail(CLG_E_CAPACITY, "%s is too small (rows %llu, payload bytes %llu)", pay_short, (unsigned long long)var->n_rows,
                (unsigned long long)var->n_var);

  // the writes
  if (!clg::pack_sizes_only(*out)) CHK(pack_write(e, pin, out));
  if (wide_any && nw) {
    for (int i = w0; i < w1; ++i)
      CHK(copy_caller(e, clg::col_ptr(*wide, i), clg::col_ptr(full, i), nw * clg::kColArray[i].width, hipMemcpyDefault,
                      wide->out_kind));
    CHK(e->sync());
  }
  if (var && ps == CLG_OK && !clg::pay_sizes_only(*var))
    ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var);
  else if (ps != CLG_OK)
    g_err = pay_err;
  if (cs != CLG_OK) {
    g_err = col_err;
    return cs;
  }
  return ps;
}

// What the decode-to-columns entry points decode, per source kind: `run` decodes it into the
// arrays it is given, `spans_of` gives its spans to the payload gather.
using DecodeRun = std::function<int(clg_decoded*, uint64_t*)>;
struct DecodeSource {
  DecodeRun run;
  std::function<int(std::vector<clg::PaySpan>&, std::vector<uint32_t>&)> spans_of;
};
DecodeRun run_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n) {
  return [=](clg_decoded* d, uint64_t* base) { return clg_decode_logs(e, log, start_epoch, n, d, base); };
}
DecodeRun run_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len, uint32_t n) {
  return [=](clg_decoded* d, uint64_t* base) { return clg_decode_host(e, bytes, span_off, span_len, n, d, base); };
}
DecodeSource source_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n) {
  return {run_logs(e, log, start_epoch, n), [=](std::vector<clg::PaySpan>& spans, std::vector<uint32_t>& segtab) {
            return payload_spans_logs(e, log, start_epoch, n, spans, segtab);
          }};
}
DecodeSource source_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                         uint32_t n) {
  return {run_host(e, bytes, span_off, span_len, n), [=](std::vector<clg::PaySpan>& spans, std::vector<uint32_t>&) {
            return payload_spans_bytes(e, bytes, span_off, span_len, n, CLG_MEM_HOST, spans);
          }};
}

}  // namespace

extern "C" {

int clg_pack_columns(clg_engine* e, const clg_columns* in, clg_packed* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::pack_reset_result(out);
  CHK(pack_out_check(*out));
  clg::PackSrc src = clg::pack_src(*in);
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    if (src.n[c] && !src.col[c]) return fail(CLG_E_INVALID_ARG, "null input array (stream %u)", c);
  if (!mem_kind_ok(in->out_kind)) return fail(CLG_E_INVALID_ARG, "the columns' out_kind %u", in->out_kind);
  PlaceSpec ins[clg::kPackStreams];
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) ins[c] = {src.col[c], src.n[c] * clg::pack_elem(c), clg::pack_elem(c)};
  clg::Placement pl;
  const int st = place_in(e, e->d_packin, ins, clg::kPackStreams, in->out_kind, PlacePolicy::stage_if_unresolved, "stream", &pl);
  if (st != CLG_OK) return clg::pack_layout(src.n, out), st;  // (a misaligned stream: the layout is filled, as pack_sizes fills it)
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) src.col[c] = pl.at<const void>(c);
  clg::PackIn pin{};
  CHK(pack_sizes(e, src, out, &pin));
  if (clg::pack_sizes_only(*out)) return CLG_OK;
  if (const char* name = clg::pack_short(*out)) return pack_capacity_error(*out, name);
  return pack_write(e, pin, out);
}

int clg_decode_logs_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                   clg_columns* wide, clg_payloads* var, clg_packed* out) {
  ENGINE_GUARD(e);
  if (!wide || !out || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_logs(e, log, start_epoch, n);
  return decode_columns_packed(e, src.run, n, wide, var, out, src.spans_of);
}

int clg_decode_host_columns_packed(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                   const uint64_t* span_len, uint32_t n, clg_columns* wide, clg_payloads* var,
                                   clg_packed* out) {
  ENGINE_GUARD(e);
  if (!wide || !out || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_host(e, bytes, span_off, span_len, n);
  return decode_columns_packed(e, src.run, n, wide, var, out, src.spans_of);
}

int clg_pack_columns_host(const clg_columns* in, clg_packed* out) {
  const char* what = "";
  const int st = clg::pack_build_host(in, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "packed columns: %s", what);
}

int clg_unpack_columns_host(const clg_packed* in, uint32_t stream, uint64_t first, uint64_t count, void* out) {
  const char* what = "";
  const int st = clg::pack_unpack_host(in, stream, first, count, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack columns: %s", what);
}

int clg_gather_payloads(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                        uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len,
                        const uint64_t* row_base, uint32_t in_kind, clg_payloads* out) {
  ENGINE_GUARD(e);
  if (!out || (n_spans && (!span_off || !span_len || !row_base))) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::pay_reset_result(out);
  if (in_kind != CLG_MEM_HOST && in_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "in_kind %u", in_kind);
  if (!clg::pay_row_base_ok(row_base, n_spans)) return fail(CLG_E_INVALID_ARG, "row_base does not start at 0 or decreases");
  std::vector<clg::PaySpan> spans;
  CHK(payload_spans_bytes(e, bytes, span_off, span_len, n_spans, in_kind, spans));
  const uint32_t *d_off, *d_len;
  CHK(stage_payload_rows(e, w_var_off, w_var_len, n_spans ? row_base[n_spans] : 0, in_kind, &d_off, &d_len));
  return gather_payloads_device(e, spans, {}, d_off, d_len, row_base, out);
}

int clg_gather_payloads_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                             const uint32_t* w_var_off, const uint32_t* w_var_len, const uint64_t* row_base,
                             uint32_t in_kind, clg_payloads* out) {
  ENGINE_GUARD(e);
  if (!out || (n && (!log || !start_epoch || !row_base))) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::pay_reset_result(out);
  if (in_kind != CLG_MEM_HOST && in_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "in_kind %u", in_kind);
  if (!clg::pay_row_base_ok(row_base, n)) return fail(CLG_E_INVALID_ARG, "row_base does not start at 0 or decreases");
  std::vector<clg::PaySpan> spans;
  std::vector<uint32_t> segtab;
  CHK(payload_spans_logs(e, log, start_epoch, n, spans, segtab));
  const uint32_t *d_off, *d_len;
  CHK(stage_payload_rows(e, w_var_off, w_var_len, n ? row_base[n] : 0, in_kind, &d_off, &d_len));
  return gather_payloads_device(e, spans, segtab, d_off, d_len, row_base, out);
}

int clg_decode_logs_columns_var(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                clg_columns* out, clg_payloads* var) {
  ENGINE_GUARD(e);
  if (!out || !var || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_logs(e, log, start_epoch, n);
  return decode_columns_var(e, src.run, n, out, var, src.spans_of);
}

int clg_decode_host_columns_var(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                const uint64_t* span_len, uint32_t n, clg_columns* out, clg_payloads* var) {
  ENGINE_GUARD(e);
  if (!out || !var || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  // The bytes are staged again: the decode's staged copy shares d_stage with its fallbacks'
  // re-plans, so whether it is intact when the decode returns depends on the path the decode took.
  const DecodeSource src = source_host(e, bytes, span_off, span_len, n);
  return decode_columns_var(e, src.run, n, out, var, src.spans_of);
}

int clg_gather_payloads_host(const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                             uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len,
                             const uint64_t* row_base, clg_payloads* out) {
  const char* what = "";
  const int st = clg::pay_build_host(bytes, span_off, span_len, n_spans, w_var_off, w_var_len, row_base, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "payloads: %s", what);
}

int clg_columnize(clg_engine* e, const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans,
                  clg_columns* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  if (in->out_kind != CLG_MEM_DEVICE && in->out_kind != CLG_MEM_MAPPED)  // (host input is not staged here)
    return fail(CLG_E_INVALID_ARG, "the decoded batch must be device or registered memory (out_kind %u)", in->out_kind);
  clg_decoded d = *in;
  // registered host memory: its device side.  (Element size 1: the input's alignment is not checked.)
  const uint64_t n = in->n_rec, w = in->n_wide;
  const PlaceSpec ins[8] = {{d.tag, n, 1},       {d.v0, n * 8, 1},        {d.w_idx, w * 4, 1},     {d.w_rc, w * 4, 1},
                            {d.w_v1, w * 8, 1},  {d.w_var_off, w * 4, 1}, {d.w_var_len, w * 4, 1}, {d.w_sub, w, 1}};
  clg::Placement pl;
  CHK(place_arrays(ins, 8, in->out_kind, PlacePolicy::reject_unresolved, "input", &pl));
  d.tag = pl.at<uint8_t>(0), d.v0 = pl.at<int64_t>(1), d.w_idx = pl.at<uint32_t>(2), d.w_rc = pl.at<int32_t>(3);
  d.w_v1 = pl.at<int64_t>(4), d.w_var_off = pl.at<uint32_t>(5), d.w_var_len = pl.at<uint32_t>(6), d.w_sub = pl.at<uint8_t>(7);
  return columnize_device(e, d, span_rec_base, n_spans, out);
}

int clg_decode_logs_columns(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                            clg_columns* out) {
  ENGINE_GUARD(e);
  if (!out || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  return decode_columns(e, run_logs(e, log, start_epoch, n), n, out);
}

int clg_decode_host_columns(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                            uint32_t n, clg_columns* out) {
  ENGINE_GUARD(e);
  if (!out || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  return decode_columns(e, run_host(e, bytes, span_off, span_len, n), n, out);
}

int clg_columnize_host(const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans, clg_columns* out) {
  const char* what = "";
  const int st = clg::col_build_host(in, span_rec_base, n_spans, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "columns: %s", what);
}

int clg_replay_prep(clg_engine* e, const uint64_t* key, const uint8_t* bytes, const uint64_t* off, const uint64_t* len,
                    uint32_t n, uint32_t* winner, uint32_t* n_keys, clg_decoded* out, uint64_t* span_rec_base) {
  ENGINE_GUARD(e);
  if (n && (!key || !off || !len || !winner || !n_keys)) return fail(CLG_E_INVALID_ARG, "null argument");
  // DeterminantResponseEvent.merge :136-146: per CausalLogID keep the longer buffer,
  // ties -> the later one (v2).  Keys keep first-appearance order.
  std::unordered_map<uint64_t, uint32_t> best;
  std::vector<uint64_t> order;
  for (uint32_t i = 0; i < n; ++i) {
    auto it = best.find(key[i]);
    if (it == best.end()) {
      best.emplace(key[i], i);
      order.push_back(key[i]);
    } else if (!(len[it->second] > len[i])) {
      it->second = i;
    }
  }
  *n_keys = uint32_t(order.size());
  std::vector<uint64_t> so(order.size()), sl(order.size());
  for (size_t k = 0; k < order.size(); ++k) {
    winner[k] = best[order[k]];
    so[k] = off[winner[k]];
    sl[k] = len[winner[k]];
  }
  if (!out) return CLG_OK;
  return clg_decode_host(e, bytes, so.data(), sl.data(), uint32_t(order.size()), out, span_rec_base);
}

}  // extern "C"

// ReplayingState (:58-66, :108-130) + SubpartitionRecoveryThread.run (:157-188) +
// LogReplayerImpl (:51-158), batched over failed vertices.  Main logs go through the
// batched decode; subpartition recovery buffers through k_bufsizes (5-byte BufferBuilt
// records, no chain walk).  All inputs are staged to HBM in one copy.
//
// replay_prepare is both forms' lookup, staging, subpartition kernels and outputs; only the
// main-log step differs: `main(build, main_bytes, staged)` decodes the main logs (span i = vertex
// i) from the plan `build` fills over the staged bytes, whose places `staged` gives as contiguous
// PaySpans.  finish_sub: a main step that fails does not end the call before the subpartition
// outputs are delivered (the columns form: a decode error is a result there); its status is the
// call's.
namespace {
struct ReplaySubOut {  // clg_replay_out's subpartition fields
  int32_t* buffer_sizes;
  uint64_t sizes_cap;
  uint64_t* sizes_base;
  uint64_t* sub_count;
  int32_t* sub_status;
  int64_t* sub_err_off;
  int32_t* sub_err_tag;
};
using ReplayBuild = clg_engine::PlanBuild;
using ReplayMain = std::function<int(const ReplayBuild&, uint64_t, const std::vector<clg::PaySpan>&)>;
}  // namespace
static int replay_prepare(clg_engine* e, const clg_replay_vertex* v, uint32_t n, const ReplaySubOut* out, bool dev_in,
                          bool finish_sub, const ReplayMain& main);
static int replay_prepare_soa(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out, bool dev_in) {
  ENGINE_GUARD(e);
  if (!out || !out->main || !out->main_rec_base || (n && !v)) return fail(CLG_E_INVALID_ARG, "null argument");
  const ReplaySubOut so{out->buffer_sizes, out->sizes_cap,   out->sizes_base, out->sub_count,
                        out->sub_status,   out->sub_err_off, out->sub_err_tag};
  return replay_prepare(e, v, n, &so, dev_in, false,
                        [&](const ReplayBuild& build, uint64_t main_bytes, const std::vector<clg::PaySpan>&) {
                          return e->decode(build, main_bytes, out->main, out->main_rec_base);
                        });
}

extern "C" {

int clg_replay_prepare(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out) {
  return replay_prepare_soa(e, v, n, out, false);
}
int clg_replay_prepare_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out) {
  return replay_prepare_soa(e, v, n, out, true);
}

}  // extern "C"

// The columns form: the main step is the decode into engine scratch, the columns of what it
// produced, and (var set) the payload column of the wide rows, gathered from the bytes where
// replay_prepare staged them.  They are not staged a second time: d_stage has two writers,
// flush() and stage_spans(), and neither runs between the staging and the payload gather -- the
// decode and its fallbacks re-plan at the same addresses, the column kernels do not touch it, and
// the spans handed to the gather are contiguous device memory already (no payload_spans_bytes).
static int replay_prepare_columns(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_columns_out* out,
                                  bool dev_in) {
  ENGINE_GUARD(e);
  if (!out || !out->main || (n && !v)) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::col_reset_result(out->main);
  if (out->var) clg::pay_reset_result(out->var);
  const ReplaySubOut so{out->buffer_sizes, out->sizes_cap,   out->sizes_base, out->sub_count,
                        out->sub_status,   out->sub_err_off, out->sub_err_tag};
  return replay_prepare(
      e, v, n, &so, dev_in, true, [&](const ReplayBuild& build, uint64_t main_bytes, const std::vector<clg::PaySpan>& staged) {
        const auto run = [&](clg_decoded* d, uint64_t* base) { return e->decode(build, main_bytes, d, base); };
        if (!out->var) return decode_columns(e, run, n, out->main);
        return decode_columns_var(e, run, n, out->main, out->var, [&](std::vector<clg::PaySpan>& spans, std::vector<uint32_t>&) {
          spans = staged;
          return CLG_OK;
        });
      });
}

extern "C" {

int clg_replay_prepare_columns(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_columns_out* out) {
  return replay_prepare_columns(e, v, n, out, false);
}
int clg_replay_prepare_columns_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_columns_out* out) {
  return replay_prepare_columns(e, v, n, out, true);
}

}  // extern "C"

// Pinned read-back of replay-prep's subpartition results: sizes, then count, err_off (8 B
// each), status, err_tag (4 B each) per subpartition, as they lie on the device.
static size_t o_rout_cnt(uint64_t n_sizes) { return (size_t(n_sizes) * 4 + 15) & ~size_t(15); }
static size_t o_rout_end(uint32_t ns, uint64_t n_sizes) { return o_rout_cnt(n_sizes) + size_t(ns) * 24 + 64; }
static int replay_prepare(clg_engine* e, const clg_replay_vertex* v, uint32_t n, const ReplaySubOut* out, bool dev_in,
                          bool finish_sub, const ReplayMain& main) {
  clg_engine::HostTimer lap(e, "host_replay_rest");  // (laps below: the sections)
  struct Piece {
    const uint8_t* p;
    uint64_t len;
  };
  std::vector<Piece> mains(n), subs;
  // the accumulated map's entries by CausalLogID (equals :128-149), per vertex: an
  // open-addressing table, O(entries + subpartitions) (a std::map took 0.16 ms for config 5's
  // 16 vertices x 129 entries)
  std::vector<IdKey> keys;
  std::vector<uint32_t> slot;  // entry index + 1 (0: empty)
  uint64_t mask = 0;
  const clg_response* indexed = nullptr;
  auto hkey = [](const IdKey& k) {  // splitmix64 finaliser over the fields (a vertex's keys differ in sub only)
    auto mix = [](uint64_t z) {
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      return z ^ (z >> 31);
    };
    return mix(mix(uint64_t(uint16_t(k.v)) | uint64_t(k.main) << 16 | (uint64_t(uint8_t(k.sub)) << 24 ^ uint64_t(k.lo))) ^
               uint64_t(k.hi));
  };
  auto same = [](const IdKey& a, const IdKey& b) {
    return a.v == b.v && a.main == b.main && a.sub == b.sub && a.lo == b.lo && a.hi == b.hi;
  };
  auto lookup = [&](const clg_response* r, const clg_causal_log_id& id) -> Piece {
    if (!r) return Piece{nullptr, 0};
    if (r != indexed) {
      uint64_t size = 16;
      while (size < 2ull * r->n) size <<= 1;
      mask = size - 1;
      slot.assign(size, 0u);
      keys.resize(r->n);
      for (uint32_t i = 0; i < r->n; ++i) {
        keys[i] = key_of(0, r->entries[i].id);
        uint64_t h = hkey(keys[i]) & mask;
        while (slot[h] && !same(keys[slot[h] - 1], keys[i])) h = (h + 1) & mask;
        if (!slot[h]) slot[h] = i + 1;  // the first of equal keys
      }
      indexed = r;
    }
    const IdKey k = key_of(0, id);
    for (uint64_t h = hkey(k) & mask; slot[h]; h = (h + 1) & mask)
      if (same(keys[slot[h] - 1], k)) return Piece{r->entries[slot[h] - 1].bytes, r->entries[slot[h] - 1].len};
    return Piece{nullptr, 0};
  };
  subs.reserve(1024);
  for (uint32_t i = 0; i < n; ++i) {
    if (v[i].n_subpartitions && !v[i].subpartitions) return fail(CLG_E_INVALID_ARG, "null subpartition table");
    clg_causal_log_id mid{};
    mid.vertex_id = v[i].vertex_id;
    mid.is_main = 1;
    mains[i] = lookup(v[i].acc, mid);
    for (uint32_t j = 0; j < v[i].n_subpartitions; ++j) {
      clg_causal_log_id sid = v[i].subpartitions[j];
      sid.vertex_id = v[i].vertex_id;  // id.replace(lower, upper, index) keeps the vertex (:114, :121)
      sid.is_main = 0;
      subs.push_back(lookup(v[i].acc, sid));
    }
  }
  lap.lap("host_replay_index");
  const uint32_t ns = uint32_t(subs.size());
  if (ns && (!out->sizes_base || !out->sub_count || !out->sub_status || !out->sub_err_off || !out->sub_err_tag))
    return fail(CLG_E_INVALID_ARG, "null subpartition output");
  // sizes capacity: one slot per whole 5-byte record
  uint64_t n_sizes = 0;
  for (uint32_t j = 0; j < ns; ++j) {
    out->sizes_base[j] = n_sizes;
    n_sizes += subs[j].len / 5;
  }
  if (ns) out->sizes_base[ns] = n_sizes;
  if (n_sizes > out->sizes_cap || (n_sizes && !out->buffer_sizes))
    return fail(CLG_E_CAPACITY, "buffer_sizes needs %llu entries", (unsigned long long)n_sizes);
  // stage main logs then subpartition buffers (16-byte aligned pieces) in one copy
  std::vector<uint64_t> at(n + ns);
  uint64_t total = 0, main_bytes = 0, sub_bytes = 0;
  for (uint32_t i = 0; i < n + ns; ++i) {
    const Piece& pc = i < n ? mains[i] : subs[i - n];
    at[i] = total;
    total += (pc.len + 15) & ~uint64_t(15);
    (i < n ? main_bytes : sub_bytes) += pc.len;
  }
  CHK(e->d_stage.ensure(total + 16));
  if (dev_in) {  // the winners already in HBM (e.g. an RCCL receive buffer): one device gather
    std::vector<clg::GatherPiece> pieces;
    for (uint32_t i = 0; i < n + ns; ++i) {
      const Piece& pc = i < n ? mains[i] : subs[i - n];
      for (uint64_t o = 0; o < pc.len; o += 1u << 30)  // a piece's length is 32-bit
        pieces.push_back(clg::GatherPiece{pc.p + o, at[i] + o, uint32_t(std::min<uint64_t>(pc.len - o, 1u << 30)), 0});
    }
    // (no wait: the kernels below read the staged bytes on the same stream)
    CHK(e->run_gather(pieces, total, e->d_stage.p, CLG_MEM_DEVICE, "replay_stage", false));
  } else {
    CHK(e->h_stage.ensure(total + 16));
    for (uint32_t i = 0; i < n + ns; ++i) {
      const Piece& pc = i < n ? mains[i] : subs[i - n];
      if (pc.len) memcpy(e->h_stage.as<uint8_t>() + at[i], pc.p, pc.len);
    }
    if (total) HIPCHK(hipMemcpyAsync(e->d_stage.p, e->h_stage.p, total, hipMemcpyHostToDevice, e->stream));
  }
  lap.lap("host_replay_stage");
  const uint8_t* dst = e->d_stage.as<uint8_t>();
  // subpartition buffers first (their kernels only read the staged bytes)
  std::function<int(clg::JArena)> classify;
  const int32_t* d_sub_status = nullptr;
  if (ns) {
    std::vector<clg::BufSpan> bs(ns);
    std::vector<clg::BufChunk> bc;
    constexpr uint64_t kRecPerChunk = 256;
    for (uint32_t j = 0; j < ns; ++j) {
      bs[j] = clg::BufSpan{dst + at[n + j], subs[j].len, out->sizes_base[j]};
      const uint64_t nk = (subs[j].len + 4) / 5;  // records incl. a partial tail
      for (uint64_t k = 0; k < nk; k += kRecPerChunk)
        bc.push_back(clg::BufChunk{j, 0, k, std::min(nk, k + kRecPerChunk)});
    }
    const size_t o_spans = 0, o_chunks = (ns * sizeof(clg::BufSpan) + 15) & ~size_t(15);
    const size_t o_res = (o_chunks + bc.size() * sizeof(clg::BufChunk) + 15) & ~size_t(15);
    const size_t res_bytes = size_t(ns) * (8 + 8 + 4 + 8 + 4);  // first_bad, count, status, err_off, err_tag
    CHK(e->h_rmeta.ensure(o_res + res_bytes + 64));
    CHK(e->d_rmeta.ensure(o_res + res_bytes + 64));
    uint8_t* hm = e->h_rmeta.as<uint8_t>();
    memcpy(hm + o_spans, bs.data(), ns * sizeof(clg::BufSpan));
    memcpy(hm + o_chunks, bc.data(), bc.size() * sizeof(clg::BufChunk));
    HIPCHK(hipMemcpyAsync(e->d_rmeta.p, hm, o_res, hipMemcpyHostToDevice, e->stream));
    uint8_t* dm = e->d_rmeta.as<uint8_t>();
    uint64_t* d_first = reinterpret_cast<uint64_t*>(dm + o_res);
    uint64_t* d_count = d_first + ns;
    int64_t* d_eoff = reinterpret_cast<int64_t*>(d_count + ns);
    int32_t* d_status = reinterpret_cast<int32_t*>(d_eoff + ns);
    int32_t* d_etag = d_status + ns;
    HIPCHK(hipMemsetAsync(d_first, 0xFF, ns * 8, e->stream));
    CHK(e->d_rsizes.ensure(std::max<uint64_t>(1, n_sizes) * 4));
    const auto* d_spans = reinterpret_cast<const clg::BufSpan*>(dm + o_spans);
    CHK(e->timed("replay_bufsizes", sub_bytes + 4 * n_sizes, [&] {
      return clg::launch_bufsizes(reinterpret_cast<const clg::BufChunk*>(dm + o_chunks), uint32_t(bc.size()), d_spans,
                                  e->d_rsizes.as<int32_t>(), d_first, e->stream);
    }));
    clg::JArena jar;
    CHK(e->jarena_reset(&jar));
    CHK(clg::launch_bufsizes_classify(d_spans, ns, d_first, d_count, d_status, d_eoff, d_etag, jar, e->stream));
    CHK(e->jarena_clear_note(1));
    CHK(e->jarena_note(1));
    classify = [=](clg::JArena a) {
      return clg::launch_bufsizes_classify(d_spans, ns, d_first, d_count, d_status, d_eoff, d_etag, a, e->stream);
    };
    d_sub_status = d_status;
    // read back into pinned memory (asynchronous; into the caller's pageable arrays each copy
    // was a staged synchronous one), copied out after the decode's sync below
    CHK(e->h_rout.ensure(o_rout_end(ns, n_sizes)));
    uint8_t* hr = e->h_rout.as<uint8_t>();
    if (n_sizes) HIPCHK(hipMemcpyAsync(hr, e->d_rsizes.p, n_sizes * 4, hipMemcpyDeviceToHost, e->stream));
    // count, err_off, status, err_tag: adjacent on the device (d_first's block): one copy
    HIPCHK(hipMemcpyAsync(hr + o_rout_cnt(n_sizes), d_count, size_t(ns) * 24, hipMemcpyDeviceToHost, e->stream));
  }
  lap.lap("host_replay_sizes");
  // main logs: the batched decode (span i = vertex i)
  const ReplayBuild build = [&](clg_engine::DecodePlan& p, uint32_t T) {
    for (uint32_t i = 0; i < n; ++i) e->plan_host_span(p, dst + at[i], mains[i].len, i, T);
  };
  std::vector<clg::PaySpan> staged(n);
  for (uint32_t i = 0; i < n; ++i) staged[i] = clg::PaySpan{mains[i].len ? dst + at[i] : nullptr, 0, mains[i].len, 0, 0};
  const int main_status = main(build, main_bytes, staged);
  if (main_status != CLG_OK && !finish_sub) return main_status;
  const std::string main_err = main_status != CLG_OK ? g_err : std::string();
  lap.lap("host_replay_decode");
  CHK(e->sync());
  // a Serializable walk in a subpartition buffer found the spill arena full: again, larger
  uint8_t* hr = e->h_rout.as<uint8_t>();
  const size_t oc = o_rout_cnt(n_sizes);
  while (ns && e->jarena_spilled(1)) {
    CHK(e->jarena_grow());
    clg::JArena jar;
    CHK(e->jarena_reset(&jar));
    CHK(classify(jar));
    CHK(e->jarena_note(1));
    HIPCHK(hipMemcpyAsync(hr + oc + size_t(ns) * 16, d_sub_status, size_t(ns) * 4, hipMemcpyDeviceToHost, e->stream));
    CHK(e->sync());
  }
  if (ns) {
    if (n_sizes) memcpy(out->buffer_sizes, hr, n_sizes * 4);
    memcpy(out->sub_count, hr + oc, size_t(ns) * 8);
    memcpy(out->sub_err_off, hr + oc + size_t(ns) * 8, size_t(ns) * 8);
    memcpy(out->sub_status, hr + oc + size_t(ns) * 16, size_t(ns) * 4);
    memcpy(out->sub_err_tag, hr + oc + size_t(ns) * 20, size_t(ns) * 4);
  }
  lap.lap("host_replay_finish");
  if (main_status != CLG_OK) g_err = main_err;
  return main_status;
}

extern "C" {

// SimpleDeterminantEncoder.encodeTo over a batch (encode.hip): sizes pass, one host read
// of the total, write pass.
int clg_encode_batch(clg_engine* e, const clg_encode_in* in, void* out, uint64_t cap, uint32_t out_kind,
                     uint64_t* n_out, uint64_t* bad_index) {
  ENGINE_GUARD(e);
  if (!in || !n_out || (in->n && (!in->tag || !in->v0)) ||
      (in->n_wide && (!in->w_idx || !in->w_rc || !in->w_v1 || !in->w_var_off || !in->w_var_len || !in->w_sub)) ||
      (in->var_len && !in->var))
    return fail(CLG_E_INVALID_ARG, "null argument");
  *n_out = 0;
  if (bad_index) *bad_index = UINT64_MAX;
  if (in->n == 0) return CLG_OK;
  const uint64_t n = in->n, nw = in->n_wide;
  clg::EncodeIn d{in->tag, in->v0, in->w_idx, in->w_rc, in->w_v1, in->w_var_off, in->w_var_len, in->w_sub, in->var, n, nw};
  if (in->in_kind != CLG_MEM_DEVICE) {  // stage the host arrays in one device buffer
    const size_t sz[9] = {n, 8 * n, 4 * nw, 4 * nw, 8 * nw, 4 * nw, 4 * nw, nw, size_t(in->var_len)};
    const void* src[9] = {in->tag, in->v0, in->w_idx, in->w_rc, in->w_v1, in->w_var_off, in->w_var_len, in->w_sub, in->var};
    size_t off[9], tot = 0;
    for (int i = 0; i < 9; ++i) {
      off[i] = tot;
      tot += (sz[i] + 15) & ~size_t(15);
    }
    CHK(e->d_encin.ensure(tot + 16));
    uint8_t* b = e->d_encin.as<uint8_t>();
    for (int i = 0; i < 9; ++i)
      if (sz[i]) HIPCHK(hipMemcpyAsync(b + off[i], src[i], sz[i], hipMemcpyHostToDevice, e->stream));
    d = clg::EncodeIn{b + off[0], reinterpret_cast<const int64_t*>(b + off[1]), reinterpret_cast<const uint32_t*>(b + off[2]),
                      reinterpret_cast<const int32_t*>(b + off[3]), reinterpret_cast<const int64_t*>(b + off[4]),
                      reinterpret_cast<const uint32_t*>(b + off[5]), reinterpret_cast<const uint32_t*>(b + off[6]),
                      b + off[7], b + off[8], n, nw};
  }
  const uint64_t nb = (n + 1023) / 1024;
  const size_t o_wsum = 0, o_wbase = (nb * 4 + 15) & ~size_t(15), o_bsum = o_wbase + (((nb + 1) * 8 + 15) & ~size_t(15)),
               o_bbase = o_bsum + ((nb * 8 + 15) & ~size_t(15)), o_bad = o_bbase + (((nb + 1) * 8 + 15) & ~size_t(15));
  CHK(e->d_encw.ensure(o_bad + 16));
  uint8_t* w = e->d_encw.as<uint8_t>();
  auto* wsum = reinterpret_cast<uint32_t*>(w + o_wsum);
  auto* wbase = reinterpret_cast<uint64_t*>(w + o_wbase);
  auto* bsum = reinterpret_cast<uint64_t*>(w + o_bsum);
  auto* bbase = reinterpret_cast<uint64_t*>(w + o_bbase);
  auto* bad = reinterpret_cast<uint32_t*>(w + o_bad);
  HIPCHK(hipMemsetAsync(bad, 0xFF, 4, e->stream));
  CHK(clg::launch_encode(d, wsum, wbase, bsum, bbase, bad, nullptr, 0, e->stream));
  uint64_t hres[2] = {0, 0};  // total bytes, wide rows used
  uint32_t hbad = 0;
  HIPCHK(hipMemcpyAsync(&hres[0], bbase + nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&hres[1], wbase + nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, e->stream));
  CHK(e->sync());
  if (hbad != 0xFFFFFFFFu || hres[1] != nw) {
    if (bad_index) *bad_index = hbad != 0xFFFFFFFFu ? hbad : n;
    return fail(CLG_E_INVALID_ARG, "record %llu: invalid tag or side-table row (%llu wide rows given, %llu used)",
                (unsigned long long)(hbad != 0xFFFFFFFFu ? hbad : n), (unsigned long long)nw,
                (unsigned long long)hres[1]);
  }
  *n_out = hres[0];
  if (hres[0] > cap || !out) return fail(CLG_E_CAPACITY, "encode needs %llu bytes", (unsigned long long)hres[0]);
  uint8_t* dst = static_cast<uint8_t*>(out);
  if (out_kind != CLG_MEM_DEVICE) {
    CHK(e->d_encout.ensure(hres[0] + 16));
    dst = e->d_encout.as<uint8_t>();
  }
  CHK(e->timed("encode_write", hres[0] + 9 * n + 25 * nw + in->var_len,
               [&] { return clg::launch_encode(d, wsum, wbase, bsum, bbase, bad, dst, 1, e->stream); }));
  if (out_kind != CLG_MEM_DEVICE) HIPCHK(hipMemcpyAsync(out, dst, hres[0], hipMemcpyDeviceToHost, e->stream));
  return e->sync();
}

}  // extern "C"

// ---- encode typed columns (encode_columns.h) ------------------------------------------------
namespace {

// A checked, sized encode: what the write pass needs.
struct EcolPlan {
  clg::EcolIn d{};
  uint32_t n_tiles = 0;
  const uint64_t* d_base = nullptr;
  const uint64_t* d_bbase = nullptr;
  uint64_t n_bytes = 0;
  uint64_t in_bytes = 0;  // bytes of the input arrays (for the stats)
};

int ecol_invalid(clg_encoded* out, uint32_t what, uint64_t index) {
  static const char* const kind[] = {"", "tag", "totals", "span", "row"};
  out->n_bytes = 0;
  out->bad_what = what;
  out->bad_index = index;
  return fail(CLG_E_INVALID_ARG, "encode columns: bad %s, index %llu", kind[what], (unsigned long long)index);
}

// Count, scan, bytes, scan64 and span bases, then the host's check of their results (pinned) --
// before any byte is written anywhere.  Fills out's results and, when given, sbb[ns + 1].
// dev_narrow (the packed calls): device addresses of the five narrow columns, used as they are
// whatever in_kind says of the other arrays.
int ecol_sizes(clg_engine* e, const clg_columns_in* in, clg_encoded* out, EcolPlan* p, uint64_t* sbb,
               const void* const* dev_narrow = nullptr) {
  clg::ecol_reset_result(out);
  if (!clg::ecol_args_ok(*in)) return fail(CLG_E_INVALID_ARG, "encode columns: null input array or unknown in_kind");
  const uint64_t n = in->n_rec, *nc = in->n_class, nw = nc[clg::kColWide];
  const uint32_t ns = clg::ecol_spans(*in);
  const uint64_t rows_bad = clg::ecol_span_rows_bad(*in);
  // the arrays, in EcolIn's order: bytes, and element sizes for the alignment check
  PlaceSpec ins[13] = {{in->tag, n, 1},        {in->order, nc[0], 1},  {in->timestamp, nc[1] * 8, 8}, {in->rng, nc[2] * 4, 4},
                       {in->buffer_built, nc[3] * 4, 4},                {in->w_rc, nw * 4, 4},         {in->w_v1, nw * 8, 8},
                       {in->w_var_len, nw * 4, 4},                      {in->w_sub, nw, 1},            {in->w_v0, nw * 8, 8},
                       {in->w_idx, nw * 4, 4}, {in->pos, (nw + 1) * 8, 8},                             {in->var, in->n_var, 1}};
  for (const PlaceSpec& a : ins) p->in_bytes += a.p ? a.bytes : 0;
  // registered arrays must be registered whole; host arrays are staged, an empty one too (a valid
  // address, never read).  With dev_narrow the first five take no part (no slot, no lookup, no
  // copy): they are absent from the placement, and their addresses are set behind it.
  for (int i = 0; dev_narrow && i < 5; ++i) ins[i].p = nullptr;
  const size_t sb_bytes = in->n_spans ? size_t(ns + 1) * clg::kColClasses * 8 : 0;
  clg::Placement pl;
  CHK(place_in(e, e->d_ecolin, ins, 13, in->in_kind, PlacePolicy::reject_unresolved, "encode columns: input", &pl, sb_bytes));
  for (int i = 0; dev_narrow && i < 5; ++i) pl.dev[i] = uintptr_t(dev_narrow[i]);
  const size_t o_sb = pl.staged() ? pl.total : 0;  // the span bases lie behind the staged arrays
  if (!pl.staged()) CHK(e->d_ecolin.ensure(sb_bytes + 16));
  uint8_t* din = e->d_ecolin.as<uint8_t>();
  clg::EcolIn& d = p->d;
  d = clg::EcolIn{pl.at<const uint8_t>(0),  pl.at<const int8_t>(1),   pl.at<const int64_t>(2),  pl.at<const int32_t>(3),
                  pl.at<const int32_t>(4),  pl.at<const int32_t>(5),  pl.at<const int64_t>(6),  pl.at<const uint32_t>(7),
                  pl.at<const uint8_t>(8),  pl.at<const int64_t>(9),  pl.at<const uint32_t>(10), pl.at<const uint64_t>(11),
                  pl.at<const uint8_t>(12), n, {nc[0], nc[1], nc[2], nc[3], nc[4]}, in->n_var};
  const uint64_t* d_sb = nullptr;
  if (sb_bytes && rows_bad == clg::kEcolNone) {
    HIPCHK(hipMemcpyAsync(din + o_sb, in->span_base, sb_bytes, hipMemcpyHostToDevice, e->stream));
    d_sb = reinterpret_cast<const uint64_t*>(din + o_sb);
  }

  // work: counts | class bases | byte sums | bad rows | byte bases
  const uint64_t n_tiles64 = (n + clg::kEcolTile - 1) / clg::kEcolTile;
  if (n_tiles64 > 0x7FFFFFFFull) return fail(CLG_E_INVALID_ARG, "%llu records in one call", (unsigned long long)n);
  const uint32_t nt = uint32_t(n_tiles64);
  const uint64_t wb[5] = {uint64_t(nt) * clg::kColCountWords * 4, uint64_t(nt) * clg::kColClasses * 8, uint64_t(nt) * 8,
                          uint64_t(nt) * 8, uint64_t(nt) * 8};
  size_t wo[6];
  CHK(e->d_ecolw.ensure(clg::place_layout(wb, 5, wo) + 16));
  uint8_t* wk = e->d_ecolw.as<uint8_t>();
  uint32_t* d_counts = reinterpret_cast<uint32_t*>(wk + wo[0]);
  uint64_t* d_base = reinterpret_cast<uint64_t*>(wk + wo[1]);
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(wk + wo[2]);
  uint64_t* d_bad = reinterpret_cast<uint64_t*>(wk + wo[3]);
  uint64_t* d_bbase = reinterpret_cast<uint64_t*>(wk + wo[4]);
  const size_t o_eres = clg_engine::al16(sizeof(clg::ColRes)), o_so = o_eres + clg_engine::al16(sizeof(clg::EcolRes));
  CHK(e->h_ecolres.ensure(o_so + size_t(ns + 1) * 16));
  clg::ColRes* cres = e->h_ecolres.as<clg::ColRes>();
  clg::EcolRes* eres = reinterpret_cast<clg::EcolRes*>(e->h_ecolres.as<uint8_t>() + o_eres);
  uint64_t* span_out = reinterpret_cast<uint64_t*>(e->h_ecolres.as<uint8_t>() + o_so);
  p->n_tiles = nt, p->d_base = d_base, p->d_bbase = d_bbase;

  const clg::ColIn cin{d.tag, nullptr, nullptr, n, nw};
  CHK(e->timed("encode_columns", n + 13 * nw + uint64_t(nt) * 120 + sb_bytes, [&] {
    CHK(clg::launch_col_count_scan(cin, nt, d_counts, d_base, cres, e->stream));
    return clg::launch_ecol_sizes(d, nt, d_base, d_sum, d_bad, d_bbase, cres, eres, d_sb, in->n_spans, span_out, e->stream);
  }));
  CHK(e->sync());
  if (cres->bad_tile != clg::kColNoTile) {
    CHK(clg::launch_col_find_bad(cin, cres->bad_tile, cres, e->stream));
    CHK(e->sync());
    return ecol_invalid(out, CLG_ENC_BAD_TAG, cres->bad_index);
  }
  for (uint32_t c = 0; c < clg::kColClasses; ++c)
    if (cres->total[c] != nc[c]) return ecol_invalid(out, CLG_ENC_BAD_TOTALS, c);
  if (rows_bad != clg::kEcolNone) return ecol_invalid(out, CLG_ENC_BAD_SPAN, rows_bad);
  if (d_sb)
    for (uint32_t s = 0; s <= ns; ++s)
      if (span_out[size_t(s) * 2 + 1]) return ecol_invalid(out, CLG_ENC_BAD_SPAN, s);
  if (eres->bad_row != clg::kEcolNone) return ecol_invalid(out, CLG_ENC_BAD_ROW, eres->bad_row);
  p->n_bytes = out->n_bytes = eres->n_bytes;
  for (uint32_t s = 0; s <= ns; ++s) {
    const uint64_t b = d_sb ? span_out[size_t(s) * 2] : s ? eres->n_bytes : 0;
    if (sbb) sbb[s] = b;
    if (out->span_byte_base) out->span_byte_base[s] = b;
  }
  return CLG_OK;
}

int ecol_write(clg_engine* e, const EcolPlan& p, uint8_t* d_dst) {
  return e->timed("encode_columns", p.in_bytes + uint64_t(p.n_tiles) * 48 + p.n_bytes, [&] {
    return clg::launch_ecol_write(p.d, p.n_tiles, p.d_base, p.d_bbase, p.n_bytes, d_dst, e->stream);
  });
}

// clg_encode_columns after its argument checks (the engine guard held); dev_narrow as ecol_sizes'.
int encode_columns_checked(clg_engine* e, const clg_columns_in* in, clg_encoded* out, const void* const* dev_narrow) {
  EcolPlan p;
  CHK(ecol_sizes(e, in, out, &p, nullptr, dev_narrow));
  if (!out->bytes) return CLG_OK;  // sizes only
  if (out->cap < p.n_bytes) return fail(CLG_E_CAPACITY, "encode columns needs %llu bytes", (unsigned long long)p.n_bytes);
  if (!p.n_bytes) return CLG_OK;
  // host and registered memory alike go through staging: the edge byte stores stay off the link
  const PlaceSpec dst[1] = {{out->bytes, p.n_bytes, 1}};
  clg::Placement pl;
  CHK(place_out(e->d_ecolout, dst, 1, out->out_kind, PlacePolicy::stage_unless_device, "output", &pl));
  CHK(ecol_write(e, p, pl.at<uint8_t>(0)));
  CHK(stage_out(e, dst, 1, pl));
  return e->sync();
}

int append_columns_checked(clg_engine* e, const uint32_t* log, const int64_t* epoch, const clg_columns_in* in,
                           uint64_t* span_bytes, int32_t* status, const void* const* dev_narrow);

}  // namespace

extern "C" {

int clg_encode_columns(clg_engine* e, const clg_columns_in* in, clg_encoded* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  return encode_columns_checked(e, in, out, nullptr);
}

int clg_encode_columns_host(const clg_columns_in* in, clg_encoded* out) {
  const char* what = "";
  const int st = clg::ecol_build_host(in, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "encode columns: %s", what);
}

int clg_append_columns(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                       const clg_columns_in* in, uint64_t* span_bytes, int32_t* status) {
  ENGINE_GUARD(e);
  if (!in || !log || !epoch || !status) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint32_t ns = clg::ecol_spans(*in);
  if (n_spans != ns) return fail(CLG_E_INVALID_ARG, "%u logs for %u spans", n_spans, ns);
  for (uint32_t s = 0; s < ns; ++s) status[s] = CLG_OK;
  return append_columns_checked(e, log, epoch, in, span_bytes, status, nullptr);
}

}  // extern "C"

namespace {
// clg_append_columns after its argument checks (the engine guard held, every status CLG_OK);
// dev_narrow as ecol_sizes'.
int append_columns_checked(clg_engine* e, const uint32_t* log, const int64_t* epoch, const clg_columns_in* in,
                           uint64_t* span_bytes, int32_t* status, const void* const* dev_narrow) {
  const uint32_t ns = clg::ecol_spans(*in);
  CHK(e->flush());  // pending host bytes first: the logs keep their byte order
  clg_encoded enc{};
  enc.out_kind = CLG_MEM_DEVICE;
  EcolPlan p;
  std::vector<uint64_t> sbb(size_t(ns) + 1);
  CHK(ecol_sizes(e, in, &enc, &p, sbb.data(), dev_narrow));
  for (uint32_t s = 0; s < ns && span_bytes; ++s) span_bytes[s] = sbb[s + 1] - sbb[s];
  CHK(e->d_ecolout.ensure(p.n_bytes + 16));
  CHK(ecol_write(e, p, e->d_ecolout.as<uint8_t>()));
  CHK(e->gwait());  // the scatter below writes segments an in-flight gather may read

  size_t bound = 0;
  for (uint32_t s = 0; s < ns; ++s) bound += size_t((sbb[s + 1] - sbb[s]) / e->C()) + 2;
  CHK(e->h_desc.ensure(bound * sizeof(clg::ScatterChunk)));
  clg::ScatterChunk* ch = e->h_desc.as<clg::ScatterChunk>();
  size_t nch = 0, total = 0;
  {
    std::lock_guard<std::mutex> pool_guard(e->pool_mu);
    for (uint32_t s = 0; s < ns; ++s) {  // clg_engine::append's steps, a span at a time
      const uint64_t len = sbb[s + 1] - sbb[s];
      Log* l;
      if ((status[s] = e->get_log(log[s], &l)) != CLG_OK) continue;
      if (l->depth == 0) continue;
      if (len >> 31) {
        status[s] = fail(CLG_E_INVALID_ARG, "span %u holds %llu bytes", s, (unsigned long long)len);
        continue;
      }
      if ((status[s] = e->ensure_space_locked(*l, int32_t(len))) != CLG_OK) continue;
      clg_engine::compute_if_absent(*l, epoch[s]);
      int32_t at = l->writer;
      uint64_t src = sbb[s];
      uint32_t left = uint32_t(len);
      while (left) {
        const uint32_t si = uint32_t(at) / e->C(), so = uint32_t(at) % e->C();
        const uint32_t take = std::min<uint32_t>(left, e->C() - so);
        ch[nch++] = clg::ScatterChunk{e->seg_addr(l->segs[si]) + so, src, take, e->life_word(l->segs[si], left > take)};
        at += int32_t(take);
        src += take;
        left -= take;
      }
      l->writer += int32_t(len);
      l->flushed = l->writer;
      clg_engine::reset_tail(*l);  // these bytes are in HBM only
      total += size_t(len);
    }
  }
  if (!nch) return e->sync();
  const size_t db = nch * sizeof(clg::ScatterChunk);
  CHK(e->d_desc.ensure(db));
  HIPCHK(hipMemcpyAsync(e->d_desc.p, e->h_desc.p, db, hipMemcpyHostToDevice, e->stream));
  CHK(e->timed("append_columns_scatter", 2 * total, [&] {
    return clg::launch_scatter(e->d_desc.as<clg::ScatterChunk>(), uint32_t(nch), e->d_ecolout.as<uint8_t>(), e->stream,
                               e->side_arg());
  }));
  return e->sync();  // the pinned descriptors are free again
}
}  // namespace

// ---- packed typed columns as input (pack.h, unpack.hip) --------------------------------------
// The way back in: a clg_packed is checked and unpacked on the device.  The check's verdict is
// read by the host after a sync, before the write pass is queued, so invalid input writes nothing.
namespace {

// Device addresses of a packed input that passed the host's layout check: device and registered
// memory in place, host memory (and registered memory not wholly inside one range) staged.
int unpack_input(clg_engine* e, const clg_packed* in, clg::UnpackIn* uin) {
  const uint64_t nb = in->blk_base[clg::kPackStreams], nbits = in->n_bits;
  if (nb >> 31) return fail(CLG_E_INVALID_ARG, "%llu blocks in one call", (unsigned long long)nb);
  CHK(pack_out_check(*in, "the packed input's "));
  const PlaceSpec ins[2] = {{in->desc, nb * sizeof(clg_pack_block), 8}, {in->bits, nbits, 16}};
  clg::Placement pl;
  CHK(place_in(e, e->d_unpackin, ins, 2, in->out_kind, PlacePolicy::stage_if_unresolved, "packed input", &pl));
  uin->desc = pl.at<const clg_pack_block>(0), uin->bits = pl.at<const uint8_t>(1), uin->n_bits = nbits;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) uin->n[c] = in->n_val[c];
  for (uint32_t c = 0; c <= clg::kPackStreams; ++c) uin->blk_base[c] = in->blk_base[c];
  return CLG_OK;
}

// The check pass and the host's reading of its verdict: CLG_E_INVALID_ARG with `bad` filled, or
// CLG_OK with the stream idle and nothing written anywhere yet.
int unpack_check(clg_engine* e, const clg::UnpackIn& uin, clg_unpack_bad* bad) {
  const uint64_t nb = uin.blk_base[clg::kPackStreams];
  if (!nb) return CLG_OK;
  CHK(e->d_unpackres.ensure(sizeof(clg::UnpackVerdict)));
  CHK(e->h_unpackres.ensure(sizeof(clg::UnpackVerdict)));
  clg::UnpackVerdict* res = e->h_unpackres.as<clg::UnpackVerdict>();
  // (bytes: a descriptor a block; payloads are read only where the type does not hold the range)
  CHK(e->timed("unpack_columns", nb * sizeof(clg_pack_block),
               [&] { return clg::launch_unpack_check(uin, uint32_t(nb), e->d_unpackres.as<clg::UnpackVerdict>(), e->stream); }));
  HIPCHK(hipMemcpyAsync(res, e->d_unpackres.p, sizeof(clg::UnpackVerdict), hipMemcpyDeviceToHost, e->stream));
  CHK(e->sync());
  const bool block = res->bad_block != 0;
  if (!block && !res->bad_value) return CLG_OK;
  const uint64_t blk = ~uint64_t(block ? res->bad_block : res->bad_value);
  uint32_t c = 0;
  while (c + 1 < clg::kPackStreams && blk >= uin.blk_base[c + 1]) ++c;
  clg::pack_bad_set(bad, block ? CLG_UNPACK_BAD_BLOCK : CLG_UNPACK_BAD_VALUE, c, blk - uin.blk_base[c]);
  return fail(CLG_E_INVALID_ARG, "unpack columns: %s (stream %u, block %llu)",
              block ? "malformed block descriptor" : "a value outside the stream's type", c,
              (unsigned long long)(blk - uin.blk_base[c]));
}

int unpack_write(clg_engine* e, const clg::UnpackIn& uin, const clg::UnpackOut& uout) {
  const uint64_t nb = uin.blk_base[clg::kPackStreams];
  uint64_t out_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) out_bytes += uin.n[c] * clg::pack_elem(c);
  // (bytes: the descriptors again, the payloads, the plain columns once)
  return e->timed("unpack_columns", nb * sizeof(clg_pack_block) + uin.n_bits + out_bytes,
                  [&] { return clg::launch_unpack_write(uin, uout, uint32_t(nb), e->stream); });
}

// `narrow` unpacked into engine scratch for the encode: the layout and `rest`'s totals on the
// host, the check, then the write queued on the engine's stream (the encode's kernels follow it
// there).  col[5]: the plain columns' device addresses.
int unpack_for_encode(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest, clg_unpack_bad* bad,
                      const void* col[clg::kPackStreams]) {
  clg::pack_bad_reset(bad);
  if (rest->tag || rest->order || rest->timestamp || rest->rng || rest->buffer_built)
    return fail(CLG_E_INVALID_ARG, "the narrow column pointers of `rest` must be NULL: those columns are given packed");
  uint32_t stream;
  if (!clg::pack_layout_in_ok(*narrow, &stream)) {
    clg::pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
    return fail(CLG_E_INVALID_ARG, "unpack columns: blk_base, n_val, the capacities and the pointers disagree (stream %u)", stream);
  }
  const uint64_t want[clg::kPackStreams] = {rest->n_rec, rest->n_class[0], rest->n_class[1], rest->n_class[2], rest->n_class[3]};
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    if (want[c] != narrow->n_val[c]) {
      clg::pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, c, 0);
      return fail(CLG_E_INVALID_ARG, "stream %u holds %llu values, `rest` says %llu", c, (unsigned long long)narrow->n_val[c],
                  (unsigned long long)want[c]);
    }
  clg::UnpackIn uin{};
  CHK(unpack_input(e, narrow, &uin));
  uint64_t cb[clg::kPackStreams];
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) cb[c] = narrow->n_val[c] * clg::pack_elem(c);
  size_t at[clg::kPackStreams + 1];
  CHK(e->d_unpackcol.ensure(clg::place_layout(cb, clg::kPackStreams, at) + 16));
  clg::UnpackOut uout{};
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) col[c] = uout.col[c] = e->d_unpackcol.as<uint8_t>() + at[c];
  CHK(unpack_check(e, uin, bad));
  return unpack_write(e, uin, uout);
}

// `rest` with the scratch columns in place of its null narrow pointers (ecol_args_ok wants them).
clg_columns_in with_narrow(const clg_columns_in& rest, const void* const col[clg::kPackStreams]) {
  clg_columns_in full = rest;
  full.tag = static_cast<const uint8_t*>(col[0]), full.order = static_cast<const int8_t*>(col[1]);
  full.timestamp = static_cast<const int64_t*>(col[2]), full.rng = static_cast<const int32_t*>(col[3]);
  full.buffer_built = static_cast<const int32_t*>(col[4]);
  return full;
}

}  // namespace

extern "C" {

int clg_unpack_columns(clg_engine* e, const clg_packed* in, clg_columns* out, clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  bool done;
  const char* what = "";
  const int st = clg::pack_unpack_begin(in, out, bad, &done, &what);
  if (st != CLG_OK) return fail(st, "unpack columns: %s", what);
  if (done) return CLG_OK;
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  const clg::UnpackDst dst = clg::unpack_dst(*out);
  PlaceSpec outs[clg::kPackStreams];
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) outs[c] = {dst.col[c], in->n_val[c] * clg::pack_elem(c), clg::pack_elem(c)};
  clg::Placement pl;
  CHK(place_out(e->d_unpackout, outs, clg::kPackStreams, out->out_kind, PlacePolicy::stage_if_unresolved, "column", &pl));
  clg::UnpackIn uin{};
  CHK(unpack_input(e, in, &uin));
  clg::UnpackOut uout{};
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) uout.col[c] = pl.at<void>(c);
  CHK(unpack_check(e, uin, bad));
  CHK(unpack_write(e, uin, uout));
  CHK(stage_out(e, outs, clg::kPackStreams, pl));
  return e->sync();
}

int clg_unpack_columns_all_host(const clg_packed* in, clg_columns* out, clg_unpack_bad* bad) {
  const char* what = "";
  const int st = clg::pack_unpack_all_host(in, out, bad, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack columns: %s", what);
}

int clg_encode_columns_packed(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest, clg_encoded* out,
                              clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  if (!narrow || !rest || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  clg::ecol_reset_result(out);
  const void* col[clg::kPackStreams];
  CHK(unpack_for_encode(e, narrow, rest, bad, col));
  const clg_columns_in full = with_narrow(*rest, col);
  return encode_columns_checked(e, &full, out, col);
}

int clg_append_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                              const clg_packed* narrow, const clg_columns_in* rest, uint64_t* span_bytes, int32_t* status,
                              clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  if (!narrow || !rest || !log || !epoch || !status) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint32_t ns = clg::ecol_spans(*rest);
  if (n_spans != ns) return fail(CLG_E_INVALID_ARG, "%u logs for %u spans", n_spans, ns);
  for (uint32_t s = 0; s < ns; ++s) status[s] = CLG_OK;
  const void* col[clg::kPackStreams];
  CHK(unpack_for_encode(e, narrow, rest, bad, col));
  const clg_columns_in full = with_narrow(*rest, col);
  return append_columns_checked(e, log, epoch, &full, span_bytes, status, col);
}

}  // extern "C"

namespace {
void wr16(std::vector<uint8_t>& b, uint16_t v) { b.push_back(uint8_t(v >> 8)); b.push_back(uint8_t(v)); }
void wr32(std::vector<uint8_t>& b, uint32_t v) { wr16(b, uint16_t(v >> 16)); wr16(b, uint16_t(v)); }
void wr64(std::vector<uint8_t>& b, uint64_t v) { wr32(b, uint32_t(v >> 32)); wr32(b, uint32_t(v)); }
uint32_t rd32(const uint8_t* p) { return uint32_t(p[0]) << 24 | uint32_t(p[1]) << 16 | uint32_t(p[2]) << 8 | p[3]; }
uint64_t rd64(const uint8_t* p) { return uint64_t(rd32(p)) << 32 | rd32(p + 4); }
}  // namespace

extern "C" {

// enrichWithCausalLogDelta (AbstractDeltaSerializerDeserializer.java:89-115) for a batch of
// channels: host metadata (hasDelta / offset / take) and header bytes, then one gather
// kernel writes headers and deltas into the output.
int clg_enrich_batch(clg_engine* e, uint32_t strategy, clg_enrich_req* reqs, uint32_t n, const uint32_t* log,
                     const uint8_t* flags, void* out, uint64_t cap, uint32_t out_kind, uint64_t* total) {
  ENGINE_GUARD(e);
  if ((n && (!reqs || !log)) || !total || strategy > CLG_DELTA_HIERARCHICAL)
    return fail(CLG_E_INVALID_ARG, "null argument or unknown strategy");
  CHK(e->flush());
  struct Adv {
    uint32_t log;
    ChKey k;
    int32_t nb;
  };
  struct Sent {
    uint32_t log;
    int32_t phys, nb;
    uint64_t dst;
  };
  std::vector<Adv> advs;
  std::vector<Sent> sent;
  std::vector<uint8_t> hdr;          // all headers back to back
  std::vector<uint64_t> hdr_at(n);   // request -> its header offset in hdr
  uint64_t dst = 0;
  for (uint32_t i = 0; i < n; ++i) {
    clg_enrich_req& r = reqs[i];
    r.status = CLG_OK;
    r.out_off = dst;
    const ChKey k{r.consumer.lo, r.consumer.hi};
    const size_t h0 = hdr.size();
    hdr_at[i] = h0;
    wr32(hdr, 0);  // header size, patched below (:98, :103)
    wr64(hdr, uint64_t(r.epoch));
    uint64_t dlen = 0;
    auto one = [&](uint32_t j, bool* has_out, int32_t* ofe, int32_t* nb) -> int {  // hasDelta, then take if sent
      int32_t has = 0;
      *has_out = false;
      CHK(e->has_delta(log[j], k, r.epoch, &has));
      if (!has || !(flags ? (flags[j] & CLG_DE_SEND) : 1)) return CLG_OK;
      CHK(e->offset_from_epoch(log[j], k, ofe));
      int32_t phys;
      CHK(e->take_delta(log[j], k, r.epoch, &phys, nb));
      advs.push_back(Adv{log[j], k, *nb});
      sent.push_back(Sent{log[j], phys, *nb, dlen});  // dst relative to the request's deltas, fixed below
      dlen += uint64_t(*nb);
      *has_out = true;
      return CLG_OK;
    };
    const size_t sent0 = sent.size();
    int st = CLG_OK;
    if (strategy == CLG_DELTA_FLAT) {  // [CausalLogID][offsetFromEpoch i32][len i32] per sent log (:80-84, :91-99)
      for (uint32_t j = r.first; j < r.first + r.count && st == CLG_OK; ++j) {
        bool has;
        int32_t ofe = 0, nb = 0;
        st = one(j, &has, &ofe, &nb);
        if (st != CLG_OK || !has) continue;
        const clg_causal_log_id& id = e->logs[log[j]].id;
        wr16(hdr, uint16_t(id.vertex_id));
        hdr.push_back(id.is_main ? 1 : 0);
        if (!id.is_main) {
          wr64(hdr, uint64_t(id.irp_lower));
          wr64(hdr, uint64_t(id.irp_upper));
          hdr.push_back(uint8_t(id.subpartition));
        }
        wr32(hdr, uint32_t(ofe));
        wr32(hdr, uint32_t(nb));
      }
    } else {  // Grouping: per vertex [vertex i16][hasMain]{main}[numPartitions u8]{[lo][hi][numSub u8]{[sub][ofe][len]}}
      uint32_t j = r.first;
      const uint32_t end = r.first + r.count;
      while (j < end && st == CLG_OK) {
        const int16_t v = e->logs[log[j]].id.vertex_id;
        const size_t vstart = hdr.size();
        int updates = 0;
        wr16(hdr, uint16_t(v));  // :113-115
        bool has = false;
        int32_t ofe = 0, nb = 0;
        if (e->logs[log[j]].id.is_main) {  // :116-121
          st = one(j, &has, &ofe, &nb);
          ++j;
        }
        if (st != CLG_OK) break;
        hdr.push_back(has ? 1 : 0);
        if (has) {
          wr32(hdr, uint32_t(ofe));
          wr32(hdr, uint32_t(nb));
          ++updates;
        }
        const size_t np_at = hdr.size();
        hdr.push_back(0);  // numPartitionDeltas (:134-141)
        int parts = 0;
        while (j < end && st == CLG_OK && e->logs[log[j]].id.vertex_id == v && !e->logs[log[j]].id.is_main) {
          const int64_t lo = e->logs[log[j]].id.irp_lower, hi = e->logs[log[j]].id.irp_upper;
          const size_t pstart = hdr.size();
          wr64(hdr, uint64_t(lo));  // :146-148
          wr64(hdr, uint64_t(hi));
          const size_t ns_at = hdr.size();
          hdr.push_back(0);
          int subs = 0;
          while (j < end && e->logs[log[j]].id.vertex_id == v && !e->logs[log[j]].id.is_main &&
                 e->logs[log[j]].id.irp_lower == lo && e->logs[log[j]].id.irp_upper == hi) {
            bool hs;
            int32_t o2 = 0, n2 = 0;
            st = one(j, &hs, &o2, &n2);
            if (st != CLG_OK) break;
            if (hs) {  // :150-154
              hdr.push_back(uint8_t(e->logs[log[j]].id.subpartition));
              wr32(hdr, uint32_t(o2));
              wr32(hdr, uint32_t(n2));
              ++subs;
            }
            ++j;
          }
          if (subs == 0) {
            hdr.resize(pstart);  // :156-158
          } else {
            hdr[ns_at] = uint8_t(subs);
            ++parts;
          }
        }
        hdr[np_at] = uint8_t(parts);
        updates += parts;
        if (updates == 0) hdr.resize(vstart);  // :125-126
        if (j < end && st == CLG_OK && e->logs[log[j]].id.vertex_id != v) continue;
        if (j < end && st == CLG_OK && e->logs[log[j]].id.vertex_id == v && e->logs[log[j]].id.is_main) {
          st = fail(CLG_E_INVALID_ARG, "hierarchical entries: vertex %d repeats", int(v));
        }
      }
    }
    if (st != CLG_OK) {  // undo this request's takes; the request reports the error
      for (size_t q = sent0; q < sent.size(); ++q) e->logs[sent[q].log].consumers[k].offset -= sent[q].nb;
      advs.resize(advs.size() - (sent.size() - sent0));
      sent.resize(sent0);
      hdr.resize(h0);
      r.status = st;
      r.header_bytes = 0;
      r.out_len = 0;
      continue;
    }
    const uint32_t hb = uint32_t(hdr.size() - h0);
    hdr[h0] = uint8_t(hb >> 24), hdr[h0 + 1] = uint8_t(hb >> 16), hdr[h0 + 2] = uint8_t(hb >> 8), hdr[h0 + 3] = uint8_t(hb);
    for (size_t q = sent0; q < sent.size(); ++q) sent[q].dst += dst + hb;
    r.header_bytes = hb;
    r.out_len = hb + dlen;
    dst += r.out_len;
  }
  *total = dst;
  if (dst > cap || (dst && !out)) {  // nothing moves: undo every take
    for (auto& a : advs) e->logs[a.log].consumers[a.k].offset -= a.nb;
    return fail(CLG_E_CAPACITY, "enrich needs %llu bytes", (unsigned long long)dst);
  }
  if (dst == 0) return CLG_OK;
  // headers staged in HBM (guard bytes either side for the gather's aligned reads)
  constexpr size_t kG = 32;
  CHK(e->d_hdr.ensure(hdr.size() + 2 * kG));
  CHK(e->h_stage.ensure(hdr.size() + 16));
  memcpy(e->h_stage.p, hdr.data(), hdr.size());
  uint8_t* dh = e->d_hdr.as<uint8_t>() + kG;
  HIPCHK(hipMemcpyAsync(dh, e->h_stage.p, hdr.size(), hipMemcpyHostToDevice, e->stream));
  std::vector<clg::GatherPiece> pieces;
  for (uint32_t i = 0; i < n; ++i)
    if (reqs[i].status == CLG_OK && reqs[i].header_bytes)
      pieces.push_back(clg::GatherPiece{dh + hdr_at[i], reqs[i].out_off, reqs[i].header_bytes, 0});
  for (auto& q : sent)
    if (q.nb > 0) e->add_pieces(e->logs[q.log], q.phys, q.nb, q.dst, pieces);
  return e->run_gather(pieces, dst, out, out_kind);
}

// processCausalLogDelta (:117-163): header parsed on the host, deltas applied by the
// batched upstream scatter straight from the message buffer.
int clg_process_delta(clg_engine* e, uint32_t job, uint32_t strategy, const uint8_t* msg, uint64_t n,
                      uint32_t in_kind, int64_t* epoch, uint32_t* handles, uint32_t cap, uint32_t* n_logs,
                      uint64_t* consumed) {
  ENGINE_GUARD(e);
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  if (!msg || !epoch || !n_logs || strategy > CLG_DELTA_HIERARCHICAL) return fail(CLG_E_INVALID_ARG, "null argument");
  *n_logs = 0;
  if (n < 12) return fail(CLG_E_TRUNCATED, "delta header truncated");
  std::vector<uint8_t> hb(12);
  if (in_kind == CLG_MEM_DEVICE) HIPCHK(hipMemcpy(hb.data(), msg, 12, hipMemcpyDeviceToHost));
  else memcpy(hb.data(), msg, 12);
  const int32_t hsize = int32_t(rd32(hb.data()));
  if (hsize < 12 || uint64_t(hsize) > n) return fail(CLG_E_TRUNCATED, "delta header size %d", hsize);
  hb.resize(size_t(hsize));
  if (in_kind == CLG_MEM_DEVICE) HIPCHK(hipMemcpy(hb.data(), msg, size_t(hsize), hipMemcpyDeviceToHost));
  else memcpy(hb.data(), msg, size_t(hsize));
  *epoch = int64_t(rd64(hb.data() + 4));
  size_t p = 12;
  uint64_t delta_at = uint64_t(hsize);
  std::vector<clg_delta_req> reqs;
  auto need = [&](size_t k) { return p + k <= size_t(hsize); };
  auto apply = [&](const clg_causal_log_id& id) -> int {  // processThreadDelta :129-163
    if (!need(8)) return fail(CLG_E_TRUNCATED, "delta record truncated");
    const int32_t ofe = int32_t(rd32(&hb[p])), len = int32_t(rd32(&hb[p + 4]));
    p += 8;
    if (len < 0 || delta_at + uint64_t(len) > n) return fail(CLG_E_TRUNCATED, "delta past the message");
    uint32_t h;
    const IdKey key = key_of(job, id);
    auto it = e->by_id.find(key);
    if (it == e->by_id.end()) {
      CHK(clg_log_open(e, job, &id, &h));  // insertNewUpstreamLog
    } else {
      h = it->second;
    }
    reqs.push_back(clg_delta_req{h, ofe, *epoch, delta_at, uint32_t(len), 0});
    delta_at += uint64_t(len);
    if (*n_logs < cap && handles) handles[*n_logs] = h;
    ++*n_logs;
    return CLG_OK;
  };
  while (p < size_t(hsize)) {
    clg_causal_log_id id{};
    if (!need(3)) return fail(CLG_E_TRUNCATED, "CausalLogID truncated");
    id.vertex_id = int16_t(uint16_t(hb[p]) << 8 | hb[p + 1]);
    const bool main = hb[p + 2] != 0;
    p += 3;
    if (strategy == CLG_DELTA_FLAT) {  // deserializeCausalLogID (Flat :107-119)
      id.is_main = main ? 1 : 0;
      if (!main) {
        if (!need(17)) return fail(CLG_E_TRUNCATED, "CausalLogID truncated");
        id.irp_lower = int64_t(rd64(&hb[p]));
        id.irp_upper = int64_t(rd64(&hb[p + 8]));
        id.subpartition = int8_t(hb[p + 16]);
        p += 17;
      }
      CHK(apply(id));
    } else {  // Grouping deserializeStrategyStep :66-88
      if (main) {
        id.is_main = 1;
        CHK(apply(id));
      }
      if (!need(1)) return fail(CLG_E_TRUNCATED, "partition count truncated");
      const int np = int(int8_t(hb[p++]));
      for (int q = 0; q < np; ++q) {
        if (!need(17)) return fail(CLG_E_TRUNCATED, "partition truncated");
        clg_causal_log_id sid{};
        sid.vertex_id = id.vertex_id;
        sid.irp_lower = int64_t(rd64(&hb[p]));
        sid.irp_upper = int64_t(rd64(&hb[p + 8]));
        const int ns = int(int8_t(hb[p + 16]));
        p += 17;
        for (int t = 0; t < ns; ++t) {
          if (!need(1)) return fail(CLG_E_TRUNCATED, "subpartition truncated");
          sid.subpartition = int8_t(hb[p++]);
          CHK(apply(sid));
        }
      }
    }
  }
  if (consumed) *consumed = delta_at;
  if (reqs.empty()) return CLG_OK;
  CHK(e->upstream_batch(reqs.data(), uint32_t(reqs.size()), msg, in_kind));
  for (auto& r : reqs)
    if (r.status != CLG_OK) return fail(r.status, "processUpstreamDelta failed on log %u", r.log);
  return CLG_OK;
}

}  // extern "C"

// ---- in-flight (data) log (inflightlogging/InMemorySubpartitionInFlightLogger.java) ------
static int ifl_get(clg_engine* e, uint32_t h, InFlight** out) {
  if (h >= e->ifls.size() || !e->ifls[h].open) return fail(CLG_E_NO_LOG, "unknown in-flight log handle %u", h);
  *out = &e->ifls[h];
  return CLG_OK;
}

static void ifl_release(clg_engine* e, std::vector<IflBuf>& bufs) {  // Buffer.recycleBuffer
  for (auto& b : bufs) e->ifl_free.insert(e->ifl_free.end(), b.segs.rbegin(), b.segs.rend());
  bufs.clear();
}

extern "C" {

int clg_ifl_open(clg_engine* e, uint32_t* handle) { return clg_ifl_open_typed(e, CLG_IFL_IN_MEMORY, handle); }

int clg_ifl_open_typed(clg_engine* e, uint32_t type, uint32_t* handle) {
  ENGINE_GUARD(e);
  if (!handle) return fail(CLG_E_INVALID_ARG, "null argument");
  if (type != CLG_IFL_IN_MEMORY && type != CLG_IFL_SPILLABLE) return fail(CLG_E_INVALID_ARG, "bad in-flight log type %u", type);
  uint32_t i = 0;
  while (i < e->ifls.size() && e->ifls[i].open) ++i;
  if (i == e->ifls.size()) e->ifls.emplace_back();
  e->ifls[i] = InFlight{};
  e->ifls[i].open = true;
  e->ifls[i].type = type;
  *handle = i;
  return CLG_OK;
}

int clg_ifl_close(clg_engine* e, uint32_t h) {  // close() :90-94
  ENGINE_GUARD(e);
  InFlight* f;
  CHK(ifl_get(e, h, &f));
  for (auto& kv : f->epochs) ifl_release(e, kv.second);
  f->epochs.clear();
  f->open = false;
  return CLG_OK;
}

// log(buffer, epochID, isFinished) :44-48 -- computeIfAbsent(epoch).add(buffer), batched.
// Segments are taken for the whole batch first (all-or-nothing), then one scatter copies
// every buffer into its segments.
int clg_ifl_log_batch(clg_engine* e, const uint32_t* ifl, const int64_t* epoch, const uint64_t* off,
                      const uint32_t* len, uint32_t n, const uint8_t* bytes, uint32_t in_kind) {
  ENGINE_GUARD(e);
  if (n == 0) return CLG_OK;
  if (!ifl || !epoch || !off || !len || !bytes) return fail(CLG_E_INVALID_ARG, "null argument");
  if (in_kind != CLG_MEM_HOST && in_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "bad in_kind");
  const uint32_t C = e->ifl_C;
  size_t need = 0, total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    InFlight* f;
    CHK(ifl_get(e, ifl[i], &f));
    need += (size_t(len[i]) + C - 1) / C;
    total += len[i];
  }
  if (need > e->ifl_free.size())
    return fail(CLG_E_NOSPACE, "in-flight pool exhausted (needs %zu segments, free %zu)", need, e->ifl_free.size());
  CHK(e->gwait());  // a queued gather may still read segments that were freed and are reused now
  std::vector<clg::ScatterChunk> ch;
  ch.reserve(need);
  const uint8_t* dsrc = bytes;
  if (in_kind == CLG_MEM_HOST) {  // pack the buffers into pinned staging, one upload
    CHK(e->h_stage.ensure(total ? total : 1));
    CHK(e->d_stage.ensure(total ? total : 1));
    dsrc = e->d_stage.as<uint8_t>();
  }
  uint64_t packed = 0;
  uint32_t npe = 0;  // 1 + the first buffer whose spillable log() throws after appending
  for (uint32_t i = 0; i < n; ++i) {
    IflBuf b{{}, len[i]};
    const uint64_t src = in_kind == CLG_MEM_HOST ? packed : off[i];
    if (in_kind == CLG_MEM_HOST && len[i]) memcpy(e->h_stage.as<uint8_t>() + packed, bytes + off[i], len[i]);
    for (uint32_t o = 0; o < len[i]; o += C) {
      const uint32_t s = e->ifl_free.back();
      e->ifl_free.pop_back();
      b.segs.push_back(s);
      ch.push_back(clg::ScatterChunk{e->ifl_addr(s), src + o, std::min(C, len[i] - o), 0});
    }
    packed += len[i];
    InFlight& f = e->ifls[ifl[i]];
    f.epochs[epoch[i]].push_back(std::move(b));
    if (f.type == CLG_IFL_SPILLABLE && f.replaying) {  // :98-99
      if (!f.it.exists) {
        npe = npe ? npe : i + 1;  // currentIterator is null: notifyNewBufferAdded throws
      } else {                    // SpilledReplayIterator.notifyNewBufferAdded :262-277
        for (IflCursor* c : {&f.it.pre, &f.it.con}) {
          ++c->rem;
          c->last = std::max(c->last, epoch[i]);
        }
      }
    }
  }
  if (ch.empty())
    return npe ? fail(CLG_E_STATE, "log() of buffer %u while replaying without an iterator (NullPointerException)", npe - 1)
               : CLG_OK;
  const size_t db = ch.size() * sizeof(clg::ScatterChunk);
  CHK(e->h_desc.ensure(db));
  CHK(e->d_desc.ensure(db));
  memcpy(e->h_desc.p, ch.data(), db);
  if (in_kind == CLG_MEM_HOST)
    HIPCHK(hipMemcpyAsync(e->d_stage.p, e->h_stage.p, total, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_desc.p, e->h_desc.p, db, hipMemcpyHostToDevice, e->stream));
  CHK(e->timed("ifl_scatter", 2 * total, [&] {
    return clg::launch_scatter(e->d_desc.as<clg::ScatterChunk>(), uint32_t(ch.size()), dsrc, e->stream);
  }));
  HIPCHK(hipStreamSynchronize(e->stream));  // staging buffers are reused; device input is the caller's
  if (npe) return fail(CLG_E_STATE, "log() of buffer %u while replaying without an iterator (NullPointerException)", npe - 1);
  return CLG_OK;
}

int clg_ifl_notify_checkpoint_complete(clg_engine* e, uint32_t h, int64_t cp) {  // :51-70
  ENGINE_GUARD(e);
  InFlight* f;
  CHK(ifl_get(e, h, &f));
  for (auto it = f->epochs.begin(); it != f->epochs.end() && it->first < cp;) {
    ifl_release(e, it->second);
    it = f->epochs.erase(it);
  }
  return CLG_OK;
}

int clg_ifl_state(clg_engine* e, uint32_t h, int64_t* ids, uint32_t* nb, uint32_t cap, uint32_t* n_epochs) {
  ENGINE_GUARD(e);
  InFlight* f;
  CHK(ifl_get(e, h, &f));
  uint32_t k = 0;
  for (auto& kv : f->epochs) {
    if (k < cap) {
      if (ids) ids[k] = kv.first;
      if (nb) nb[k] = uint32_t(kv.second.size());
    }
    ++k;
  }
  if (n_epochs) *n_epochs = k;
  return CLG_OK;
}

}  // extern "C"

// ---- the spillable logger's iterator (SpilledReplayIterator.java), on host metadata ---------
// Every EpochCursor step that reads the map through the live view tailMap(view) fails (returns
// false) where the Java code throws: an epoch missing from the view (NullPointerException) or an
// offset past its buffers (IndexOutOfBoundsException).
static bool ifl_size(const InFlight& f, int64_t view, int64_t ep, int64_t* n) {  // log.get(ep).getEpochSize()
  if (ep < view) return false;
  const auto it = f.epochs.find(ep);
  if (it == f.epochs.end()) return false;
  *n = int64_t(it->second.size());
  return true;
}
static bool ifl_advance(const InFlight& f, int64_t view, IflCursor& c) {  // advanceEpochIfNeeded :353-358
  int64_t n;
  if (!ifl_size(f, view, c.ne, &n)) return false;
  if (c.off == n && c.ne != c.last) {
    ++c.ne;
    c.off = 0;
  }
  return true;
}
static bool ifl_cnext(const InFlight& f, int64_t view, IflCursor& c, const IflBuf** out) {  // next() :342-351
  if (!ifl_advance(f, view, c)) return false;
  const auto it = c.ne >= view ? f.epochs.find(c.ne) : f.epochs.end();
  if (it == f.epochs.end() || c.off < 0 || c.off >= int64_t(it->second.size())) return false;
  if (out) *out = &it->second[size_t(c.off)];
  ++c.off;
  --c.rem;
  return ifl_advance(f, view, c);
}
static bool ifl_behind(const InFlight& f, int64_t view, IflCursor& a, IflCursor& b, bool* res) {  // behind() :364-367
  if (!ifl_advance(f, view, a) || !ifl_advance(f, view, b)) return false;
  *res = a.ne < b.ne || (a.ne == b.ne && a.off < b.off);
  return true;
}
static void ifl_prefetch(const InFlight& f, IflIter& it) {  // prefetchNextBuffers :126-158 (exceptions swallowed)
  while (it.pre.rem > 0)
    if (!ifl_advance(f, it.view, it.pre) || !ifl_cnext(f, it.view, it.pre, nullptr)) return;
}

extern "C" {

// getInFlightIterator(start, ignore) and the drain of its iterator, per logger type:
//   in-memory (:73-82, ReplayIterator :114-167): walks tailMap(start) by ++currentKey, so it only
//     yields contiguous epochs from `start`; a missing key throws inside next() right after the
//     last buffer before it was taken (:156 -> :133), so that buffer is lost to the caller;
//   spillable (:126-142, SpilledReplayIterator): the iterator is the logger's current one, its
//     cursors stepped literally (above); max_buffers / CLG_IFL_CONTINUE drain it in parts.
// Iterator state is worked on in copies and committed only when the gather runs, so a sizing
// call (CLG_E_CAPACITY) changes nothing.
int clg_ifl_replay_batch(clg_engine* e, const clg_ifl_replay_req* reqs, uint32_t n, clg_ifl_replay_res* res,
                         void* out, uint64_t cap, uint32_t out_kind, uint32_t* sizes, int64_t* epochs,
                         uint64_t sizes_cap, uint64_t* total, uint64_t* total_buffers) {
  ENGINE_GUARD(e);
  if (n && (!reqs || !res)) return fail(CLG_E_INVALID_ARG, "null argument");
  if (out_kind != CLG_MEM_HOST && out_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "bad out_kind");
  struct Pick {
    const IflBuf* b;
    uint64_t dst;
  };
  struct Work {  // a spillable logger's iterator state during this call
    IflIter it;
    bool replaying;
  };
  std::map<uint32_t, Work> work;
  std::vector<Pick> picks;
  uint64_t dst = 0, nbuf = 0;
  auto take = [&](clg_ifl_replay_res& r, const IflBuf& b, int64_t ep) {
    picks.push_back(Pick{&b, dst});
    if (nbuf < sizes_cap) {
      if (sizes) sizes[nbuf] = b.len;
      if (epochs) epochs[nbuf] = ep;  // getEpoch() before this next()
    }
    dst += b.len;
    r.len += b.len;
    ++nbuf;
    ++r.n_buffers;
  };
  for (uint32_t i = 0; i < n; ++i) {
    clg_ifl_replay_res& r = res[i];
    const int64_t start = reqs[i].start_epoch;
    r = clg_ifl_replay_res{CLG_OK, 0, 0, 0, dst, 0, nbuf, start};
    InFlight* f;
    int st = ifl_get(e, reqs[i].ifl, &f);
    if (st != CLG_OK) {
      r.status = st;
      continue;
    }
    const uint64_t ign = reqs[i].ignore_buffers;
    if (f->type == CLG_IFL_SPILLABLE) {
      auto wi = work.find(reqs[i].ifl);
      if (wi == work.end()) wi = work.emplace(reqs[i].ifl, Work{f->it, f->replaying}).first;
      Work& w = wi->second;
      if (!(reqs[i].flags & CLG_IFL_CONTINUE)) {  // getInFlightIterator :126-142
        w.replaying = true;
        const auto first = f->epochs.lower_bound(start);
        if (first == f->epochs.end()) {  // tailMap empty: null (the current iterator stays)
          r.flags = CLG_IFL_NULL_ITERATOR | CLG_IFL_REPLAYING;
          continue;
        }
        IflIter it;
        it.exists = true;
        it.view = start;
        it.con.ne = first->first;
        it.con.last = f->epochs.rbegin()->first;
        for (auto jt = first; jt != f->epochs.end(); ++jt) it.con.rem += int64_t(jt->second.size());
        it.pre = it.con;
        bool ok = true;
        for (uint64_t k = 0; k < ign && ok; ++k)  // the constructor's skip :98-101
          ok = ifl_cnext(*f, it.view, it.con, nullptr) && ifl_cnext(*f, it.view, it.pre, nullptr);
        if (!ok) {  // the constructor throws: no new iterator, isReplaying stays set
          r.status = fail(CLG_E_STATE, "skip of %llu buffers fails inside the iterator's constructor",
                          (unsigned long long)ign);
          r.flags = CLG_IFL_REPLAYING;
          continue;
        }
        ifl_prefetch(*f, it);  // :123
        w.it = it;
      } else if (!w.it.exists) {
        r.status = fail(CLG_E_STATE, "no current in-flight iterator to continue");
        r.flags = w.replaying ? CLG_IFL_REPLAYING : 0u;
        continue;
      }
      IflIter& it = w.it;
      r.remaining = uint32_t(std::max<int64_t>(it.con.rem, 0));
      const uint32_t cap_n = reqs[i].max_buffers;
      bool thrown = false;
      while (it.con.rem > 0 && (cap_n == 0 || r.n_buffers < cap_n)) {  // next() :171-203
        bool bh;
        if (!ifl_behind(*f, it.view, it.con, it.pre, &bh)) {
          thrown = true;
          break;
        }
        if (!bh) {
          ifl_prefetch(*f, it);
          if (!ifl_behind(*f, it.view, it.con, it.pre, &bh) || !bh) {  // (not behind: it would wait forever)
            thrown = true;
            break;
          }
        }
        const IflBuf* b = nullptr;
        if (!ifl_advance(*f, it.view, it.con)) {  // getEpoch() :166-168
          thrown = true;
          break;
        }
        const int64_t ep = it.con.ne;
        if (!ifl_cnext(*f, it.view, it.con, &b)) {
          thrown = true;
          break;
        }
        if (it.con.rem <= 0) w.replaying = false;  // :186-193
        ifl_prefetch(*f, it);
        take(r, *b, ep);
      }
      if (thrown) r.status = CLG_E_EPOCH_GAP;
      IflCursor c = it.con;
      r.end_epoch = ifl_advance(*f, it.view, c) ? c.ne : it.con.ne;
      r.flags = w.replaying ? CLG_IFL_REPLAYING : 0u;
      continue;
    }
    if (reqs[i].max_buffers || reqs[i].flags) {
      r.status = fail(CLG_E_INVALID_ARG, "max_buffers / CLG_IFL_CONTINUE need a spillable in-flight log");
      continue;
    }
    auto it = f->epochs.find(start);
    if (it == f->epochs.end()) {  // :121-127 -- currentIterator == null, nothing left, currentKey = start
      if (ign) r.status = fail(CLG_E_STATE, "skip of %llu buffers on an empty iterator", (unsigned long long)ign);
      continue;
    }
    uint64_t tail = 0, k = 0;  // tail: numberOfBuffersLeft (:123); k: buffers before a gap
    bool gap = false;
    int64_t expect = start;
    for (auto jt = it; jt != f->epochs.end(); ++jt) {
      tail += jt->second.size();
      if (!gap && jt->first == expect) {
        k += jt->second.size();
        ++expect;
      } else {
        gap = true;
      }
    }
    const uint64_t deliver = gap ? k - 1 : k;  // buffers next() returns
    if (ign > deliver) {  // the skip loop inside getInFlightIterator throws (:78-79)
      r.status = gap ? fail(CLG_E_STATE, "skip of %llu buffers reaches an epoch gap after %llu", (unsigned long long)ign,
                            (unsigned long long)deliver)
                     : fail(CLG_E_STATE, "skip of %llu buffers past the end (%llu)", (unsigned long long)ign,
                            (unsigned long long)deliver);
      continue;
    }
    if (gap) r.status = CLG_E_EPOCH_GAP;  // the next() after the last delivered buffer throws (:156 -> :133)
    // after the last successful next() the iterator sits on the last contiguous epoch: that
    // epoch holds the final buffer (no gap) or the K-th buffer the gap swallows
    r.end_epoch = expect - 1;
    r.remaining = uint32_t(tail - ign);
    uint64_t idx = 0;
    for (auto jt = it; jt != f->epochs.end() && idx < deliver; ++jt)
      for (const IflBuf& b : jt->second) {
        if (idx >= deliver) break;
        if (idx++ < ign) continue;
        take(r, b, jt->first);
      }
  }
  if (total) *total = dst;
  if (total_buffers) *total_buffers = nbuf;
  if (dst > cap || nbuf > sizes_cap || (nbuf && !sizes) || (dst && !out))
    return fail(CLG_E_CAPACITY, "in-flight replay needs %llu bytes / %llu sizes (cap %llu / %llu)",
                (unsigned long long)dst, (unsigned long long)nbuf, (unsigned long long)cap,
                (unsigned long long)sizes_cap);
  for (auto& kv : work) {  // commit the spillable iterators
    e->ifls[kv.first].it = kv.second.it;
    e->ifls[kv.first].replaying = kv.second.replaying;
  }
  std::vector<clg::GatherPiece> pieces;
  const uint32_t C = e->ifl_C;
  for (const Pick& p : picks)
    for (size_t s = 0; s < p.b->segs.size(); ++s) {
      const uint32_t o = uint32_t(s) * C;
      pieces.push_back(clg::GatherPiece{e->ifl_addr(p.b->segs[s]), p.dst + o, std::min(C, p.b->len - o), 0});
    }
  CHK(e->flush());
  return e->run_gather(pieces, dst, out, out_kind, "ifl_gather");
}

int clg_kernel_stats(clg_engine* e, clg_kernel_stat* out, uint32_t cap, uint32_t* n) {
  ENGINE_GUARD(e);
  CHK(e->sync());
  uint32_t i = 0;
  for (auto& kv : e->stats) {
    if (i < cap) {
      memset(&out[i], 0, sizeof out[i]);
      snprintf(out[i].name, sizeof out[i].name, "%s", kv.first.c_str());
      out[i].launches = kv.second.launches;
      out[i].total_ms = kv.second.ms;
      out[i].bytes = kv.second.bytes;
    }
    ++i;
  }
  *n = i;
  return CLG_OK;
}

int clg_kernel_stats_reset(clg_engine* e) {
  ENGINE_GUARD(e);
  CHK(e->sync());
  e->stats.clear();
  return CLG_OK;
}

}  // extern "C"
