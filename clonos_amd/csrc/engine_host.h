// engine_host.h -- the engine's host-only types: the log metadata with the reference's
// semantics (epochs, segments, consumers), the in-flight log's records, the engine lock and the
// host thread pool.  No HIP here, only the standard library and the C-ABI's types, so the
// containers are also compiled and tested on their own (tests/engine_host_main.cpp).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/clonos_engine.h"

namespace clg_internal {

struct EpochStart {
  int64_t id;
  int32_t offset;
};
struct Consumer {
  std::shared_ptr<EpochStart> es;  // ConsumerOffset.epochStart (a reference, may go stale)
  int32_t offset;
};

// EpochStart objects (with their shared_ptr control blocks) come from a per-thread free
// list: a config-4 step opens an epoch in, and truncates one out of, each of 66 k logs.
template <class T>
struct EpochAlloc {
  using value_type = T;
  EpochAlloc() = default;
  template <class U>
  EpochAlloc(const EpochAlloc<U>&) {}
  struct FreeList : std::vector<void*> {  // a thread's pooled blocks go back at its exit
    ~FreeList() {
      for (void* p : *this) ::operator delete(p);
    }
  };
  static FreeList& free_list() {
    static thread_local FreeList f;
    return f;
  }
  T* allocate(size_t n) {
    auto& f = free_list();
    if (n == 1 && !f.empty()) {
      void* p = f.back();
      f.pop_back();
      return static_cast<T*>(p);
    }
    return static_cast<T*>(::operator new(n * sizeof(T)));
  }
  void deallocate(T* p, size_t n) {
    auto& f = free_list();
    if (n == 1 && f.size() < (1u << 20)) f.push_back(p);
    else ::operator delete(p);
  }
  template <class U>
  bool operator==(const EpochAlloc<U>&) const { return true; }
  template <class U>
  bool operator!=(const EpochAlloc<U>&) const { return false; }
};

// A log's epochs: epoch id -> its start offset, in id order (the reference's
// epochStartOffsets map).  A log holds few epochs between checkpoints, appended in
// increasing order, so they live in a small sorted array, the first kInline inside the Log
// itself: a config-4 step opens an epoch in, and truncates one out of, each of 66 k logs,
// and per-log work is bound by cache misses.  The offset is kept inline; the shared
// EpochStart object (Java's EpochStartOffset, which a ConsumerOffset references) exists
// only once a consumer refers to the epoch (ref()), and rebase() keeps both in step.
struct EpochEnt {
  int64_t id = 0;
  int32_t offset = 0;
  std::shared_ptr<EpochStart> shared;  // null until a ConsumerOffset refers to the epoch
};
class EpochMap {
 public:
  EpochEnt* begin() { return data(); }
  EpochEnt* end() { return data() + n_; }
  const EpochEnt* begin() const { return data(); }
  const EpochEnt* end() const { return data() + n_; }
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  EpochEnt* find(int64_t k) {
    EpochEnt* it = lower(k);
    return it != end() && it->id == k ? it : end();
  }
  const EpochEnt* find(int64_t k) const { return const_cast<EpochMap*>(this)->find(k); }
  // computeIfAbsent(k -> offset); the entry stays valid until the next insert or erase
  EpochEnt* emplace(int64_t k, int32_t offset) {
    EpochEnt* it = lower(k);
    if (it != end() && it->id == k) return it;
    const size_t i = size_t(it - begin());
    if (big_.empty() && n_ < kInline) {
      for (size_t j = n_; j > i; --j) inl_[j] = std::move(inl_[j - 1]);
      inl_[i] = EpochEnt{k, offset, nullptr};
    } else {
      if (big_.empty()) {  // spill the inline entries
        big_.reserve(2 * kInline);
        for (uint32_t j = 0; j < n_; ++j) big_.push_back(std::move(inl_[j]));
        for (auto& x : inl_) x.shared.reset();
      }
      big_.insert(big_.begin() + long(i), EpochEnt{k, offset, nullptr});
    }
    ++n_;
    return begin() + i;
  }
  // drop every epoch with id < k (checkpoint completion)
  void erase_below(int64_t k) {
    const size_t d = size_t(lower(k) - begin());
    if (!d) return;
    if (big_.empty()) {
      for (size_t j = d; j < n_; ++j) inl_[j - d] = std::move(inl_[j]);
      for (size_t j = n_ - d; j < n_; ++j) inl_[j].shared.reset();
    } else {
      big_.erase(big_.begin(), big_.begin() + long(d));
    }
    n_ -= uint32_t(d);
  }
  // every offset -= move (the shared objects too: consumers see the rebased offset)
  void rebase(int32_t move) {
    for (EpochEnt& x : *this) {
      x.offset -= move;
      if (x.shared) x.shared->offset = x.offset;
    }
  }
  // the EpochStart object a ConsumerOffset holds (created on first reference)
  static std::shared_ptr<EpochStart> ref(EpochEnt& x) {
    if (!x.shared) x.shared = std::allocate_shared<EpochStart>(EpochAlloc<EpochStart>(), EpochStart{x.id, x.offset});
    return x.shared;
  }

 private:
  static constexpr uint32_t kInline = 2;
  EpochEnt* data() { return big_.empty() ? inl_ : big_.data(); }
  const EpochEnt* data() const { return big_.empty() ? inl_ : big_.data(); }
  EpochEnt* lower(int64_t k) {
    if (n_ == 0 || end()[-1].id < k) return end();  // the common case: a new epoch
    return std::lower_bound(begin(), end(), k, [](const EpochEnt& a, int64_t b) { return a.id < b; });
  }
  uint32_t n_ = 0;
  EpochEnt inl_[kInline];
  std::vector<EpochEnt> big_;  // all entries once more than kInline were held
};

// A log's segments (Netty components), the first kInline inside the Log itself.
class SegList {
 public:
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  uint32_t operator[](size_t i) const { return data()[i]; }
  const uint32_t* begin() const { return data(); }
  const uint32_t* end() const { return data() + n_; }
  void push_back(uint32_t v) {
    if (big_.empty() && n_ < kInline) {
      inl_[n_++] = v;
      return;
    }
    if (big_.empty()) big_.assign(inl_, inl_ + n_);
    big_.push_back(v);
    ++n_;
  }
  // drop the first k (discardReadComponents)
  void erase_front(size_t k) {
    if (!k) return;
    if (big_.empty()) {
      for (size_t j = k; j < n_; ++j) inl_[j - k] = inl_[j];
    } else {
      big_.erase(big_.begin(), big_.begin() + long(k));
      if (big_.size() <= kInline) {  // back inline
        std::copy(big_.begin(), big_.end(), inl_);
        big_.clear();
        big_.shrink_to_fit();
      }
    }
    n_ -= uint32_t(k);
  }

 private:
  static constexpr uint32_t kInline = 6;
  const uint32_t* data() const { return big_.empty() ? inl_ : big_.data(); }
  uint32_t n_ = 0;
  uint32_t inl_[kInline] = {};
  std::vector<uint32_t> big_;  // all segments once more than kInline were held
};
struct ChKey {
  uint64_t lo, hi;
  bool operator==(const ChKey& o) const { return lo == o.lo && hi == o.hi; }
};
struct ChKeyHash {
  size_t operator()(const ChKey& k) const { return std::hash<uint64_t>()(k.lo * 0x9E3779B97F4A7C15ull ^ k.hi); }
};

// JobCausalLogImpl (one per job per TaskManager, JobCausalLogFactory.java:56-67): the
// job's sharing depth (ExecutionConfig.determinantSharingDepth) and its
// latestCompletedCheckpoint, whose CAS gates the fan-out of truncation (:230-246).
struct Job {
  bool open = false;
  uint64_t lo = 0, hi = 0;  // JobID (an AbstractID)
  int32_t depth = CLG_FULL_SHARING;
  int64_t latest_cp = 0;  // JobCausalLogImpl.latestCompletedCheckpoint (:92, :117)
};

struct Log {
  clg_causal_log_id id{};
  uint32_t job = 0;
  int32_t depth = CLG_FULL_SHARING;  // the owning job's sharing depth
  bool open = false;
  SegList segs;                // composite components
  int32_t writer = 0;          // visibleWriterIndex (== composite writerIndex)
  int32_t flushed = 0;         // physical bytes [0, flushed) are resident in HBM
  // Host copy of physical bytes [tail_start, writer): the staged bytes [flushed, writer)
  // plus the most recent flushed ones (clg_config.host_tail_bytes), so a slice of the log's
  // tail -- a consumer keeping up with its producer -- is served without a GPU round trip.
  // tail_start <= flushed <= writer.
  std::vector<uint8_t> tail;
  int32_t tail_start = 0;
  uint32_t pending_bytes() const { return uint32_t(writer - flushed); }
  const uint8_t* pending_data() const { return tail.data() + (flushed - tail_start); }
  EpochMap epochs;
  std::unordered_map<ChKey, Consumer, ChKeyHash> consumers;
};

// The bytes [at, at + n) of a log split at the ends of its segments of C bytes, in order:
// f(seg_index, seg_off, take, more) per chunk, `more` on all but the last.  No chunk for n == 0.
template <class F>
inline void for_each_chunk(uint32_t at, uint32_t n, uint32_t C, F&& f) {
  while (n) {
    const uint32_t si = at / C, so = at % C;
    const uint32_t take = std::min(n, C - so);
    f(si, so, take, n > take);
    at += take;
    n -= take;
  }
}
// How many chunks that is: at most n / C + 2.
inline uint32_t chunk_count(uint32_t at, uint32_t n, uint32_t C) { return n ? (at + n - 1) / C - at / C + 1 : 0u; }

// In-flight (data) log of one subpartition (InMemorySubpartitionInFlightLogger.java:28-207):
// SortedMap<epoch, List<Buffer>>; each buffer's bytes occupy whole pool segments.
struct IflBuf {
  std::vector<uint32_t> segs;
  uint32_t len;
};
// The spillable logger's replay iterator (SpilledReplayIterator.java:60-401): a consumer and a
// prefetch EpochCursor (:306-394) over the live view tailMap(view) of the epochs.
struct IflCursor {
  int64_t ne = 0;    // nextEpoch
  int64_t off = 0;   // nextEpochOffset
  int64_t last = 0;  // lastEpoch
  int64_t rem = 0;   // remaining
};
struct IflIter {
  bool exists = false;  // currentIterator != null
  int64_t view = 0;     // the tailMap's lower bound (getInFlightIterator's epochID)
  IflCursor con, pre;
};
struct InFlight {
  bool open = false;
  uint32_t type = CLG_IFL_IN_MEMORY;
  bool replaying = false;  // spillable: isReplaying (:58)
  IflIter it;              // spillable: currentIterator (:60)
  std::map<int64_t, std::vector<IflBuf>> epochs;
};

struct IdKey {  // (job, CausalLogID): logs of different jobs never alias
  uint32_t job;
  int16_t v;
  uint8_t main;
  int8_t sub;
  int64_t lo, hi;
  bool operator<(const IdKey& o) const {
    if (job != o.job) return job < o.job;
    if (v != o.v) return v < o.v;
    if (main != o.main) return main < o.main;
    if (main) return false;  // CausalLogID.equals: main logs compare by vertex only
    if (lo != o.lo) return lo < o.lo;
    if (hi != o.hi) return hi < o.hi;
    return sub < o.sub;
  }
};
inline IdKey key_of(uint32_t job, const clg_causal_log_id& id) {
  IdKey k{job, id.vertex_id, uint8_t(id.is_main ? 1 : 0), id.is_main ? int8_t(0) : id.subpartition,
          id.is_main ? 0 : id.irp_lower, id.is_main ? 0 : id.irp_upper};
  return k;
}


// Guard bytes either side of the segment pool: the gather and decode kernels issue aligned
// 16-B loads that may start before a piece's first byte or end past its last.
constexpr size_t kPoolGuard = 256;

// Two-level engine lock.  The per-call ThreadCausalLog operations of the drop-in (append,
// hasDelta, offset, slices the host tail holds, logLength, a host-input upstream delta) take
// only the stripe of their log, so task threads appending and Netty threads slicing
// different logs run in parallel -- as on the reference's per-log objects -- without
// touching a shared cache line.  Everything that touches the GPU, the log table or several
// logs at once takes the engine mutex and then every stripe (EXCLUSIVE).  Exclusive is
// re-entrant (clg_job_close -> clg_log_close), and a per-log request from the exclusive
// holder passes through.
constexpr uint32_t kLogStripes = 64;
struct alignas(64) Stripe {
  std::mutex m;
};
struct EngineLock {
  std::mutex m;
  std::atomic<std::thread::id> owner{};
  int depth = 0;
  Stripe stripe[kLogStripes];
  bool owned() const { return owner.load(std::memory_order_relaxed) == std::this_thread::get_id(); }
  void lock() {
    if (owned()) {
      ++depth;
      return;
    }
    m.lock();
    for (auto& s : stripe) s.m.lock();
    owner.store(std::this_thread::get_id(), std::memory_order_relaxed);
    depth = 1;
  }
  void unlock() {
    if (--depth == 0) {
      owner.store(std::thread::id(), std::memory_order_relaxed);
      for (uint32_t i = kLogStripes; i-- > 0;) stripe[i].m.unlock();
      m.unlock();
    }
  }
};
struct XGuard {
  EngineLock& l;
  explicit XGuard(EngineLock& l_) : l(l_) { l.lock(); }
  ~XGuard() { l.unlock(); }
};

// A few host threads for the per-log loops of very large batches (config 4: 66 k logs per
// decode, truncation): run(fn) calls fn(part, parts) once per part, the calling thread taking
// part 0; workers spin briefly for the next job, then sleep.  Jobs only ever come from the
// holder of the engine lock, one at a time.
class WorkPool {
 public:
  explicit WorkPool(unsigned n) : n_(n ? n : 1) {
    for (unsigned i = 1; i < n_; ++i) th_.emplace_back([this, i] { loop(i); });
  }
  ~WorkPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  unsigned size() const { return n_; }
  void run(const std::function<void(unsigned, unsigned)>& fn) {
    if (n_ == 1) {
      fn(0, 1);
      return;
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      job_ = &fn;
      left_.store(n_ - 1, std::memory_order_relaxed);
      gen_.fetch_add(1, std::memory_order_release);
    }
    cv_.notify_all();
    fn(0, n_);
    while (left_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
  }

 private:
  void loop(unsigned i) {
    uint64_t seen = 0;
    for (;;) {
      // a short spin (the next job of a batch comes within microseconds), then sleep: a longer
      // one burns the box's CPU quota between batches
      const auto t0 = std::chrono::steady_clock::now();
      while (gen_.load(std::memory_order_acquire) == seen &&
             std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(50))
        std::this_thread::yield();
      const std::function<void(unsigned, unsigned)>* job;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return stop_ || gen_.load(std::memory_order_acquire) != seen; });
        if (stop_) return;
        seen = gen_.load(std::memory_order_acquire);
        job = job_;
      }
      (*job)(i, n_);
      left_.fetch_sub(1, std::memory_order_acq_rel);
    }
  }
  unsigned n_;
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<unsigned> left_{0};
  const std::function<void(unsigned, unsigned)>* job_ = nullptr;
  bool stop_ = false;
};

}  // namespace clg_internal
