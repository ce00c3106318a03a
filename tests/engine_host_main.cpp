// engine_host_main.cpp -- stand-alone checks of the engine's host containers
// (clonos_amd/csrc/engine_host.h): EpochMap and SegList against std::map / std::vector models
// over random operations, EpochAlloc across threads, EngineLock, WorkPool; and of the split of a
// byte range at segment ends (for_each_chunk, chunk_count) against a byte-by-byte model.  Built by
// tests/test_engine_host.py with the address + undefined-behaviour sanitizers and again with
// the thread sanitizer; exits 0 and writes nothing to stderr when all holds.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "../clonos_amd/csrc/engine_host.h"

using namespace clg_internal;

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

#if defined(__SANITIZE_THREAD__)
// The exclusive EngineLock holds its mutex and all 64 stripes, 65 locks: the thread sanitizer's
// lock-order (deadlock) detector tracks at most 64 held by one thread and stops the program
// past that.  Only that detector is off; data races are reported as usual.
extern "C" const char* __tsan_default_options() { return "detect_deadlocks=0"; }
#endif

// ---------------------------------------------------------------- EpochMap
// A ConsumerOffset's reference to an epoch: live while the epoch is in the map (its offset
// follows every rebase), stale once erase_below dropped the epoch (its last offset stays).
struct Held {
  std::shared_ptr<EpochStart> es;
  int64_t id;
  int32_t want;
  bool live;
};

static void check_epochs(EpochMap& m, const std::map<int64_t, int32_t>& model, const std::vector<Held>& held) {
  REQUIRE(m.size() == model.size());
  REQUIRE(m.empty() == model.empty());
  REQUIRE(size_t(m.end() - m.begin()) == model.size());
  auto it = model.begin();
  for (const EpochEnt& x : m) {
    REQUIRE(x.id == it->first && x.offset == it->second);
    if (x.shared) REQUIRE(x.shared->id == x.id && x.shared->offset == x.offset);
    ++it;
  }
  const EpochMap& cm = m;
  for (const auto& kv : model) {
    REQUIRE(m.find(kv.first) != m.end() && m.find(kv.first)->offset == kv.second);
    REQUIRE(cm.find(kv.first) != cm.end() && cm.find(kv.first)->id == kv.first);
  }
  for (const Held& h : held) {
    REQUIRE(h.es->id == h.id && h.es->offset == h.want);
    if (h.live) REQUIRE(m.find(h.id) != m.end() && m.find(h.id)->shared == h.es);
    // owners: the consumers that hold it, and the map while the epoch is in it (a dropped
    // epoch's slot lets go of the object)
    long owners = h.live ? 1 : 0;
    for (const Held& o : held) owners += o.es == h.es;
    REQUIRE(h.es.use_count() == owners);
  }
}

static void test_epoch_map(uint32_t seed, int steps) {
  std::mt19937 rng(seed);
  auto rnd = [&](int n) { return int(rng() % uint32_t(n)); };
  EpochMap m;
  std::map<int64_t, int32_t> model;
  std::vector<Held> held;
  const int64_t base = 1000;
  bool seen[5] = {};  // sizes 0, 1, 2, 3, more
  bool spilled = false;
  int emptied_after_spill = 0, kept = 0, stale_checked = 0;
  for (int s = 0; s < steps; ++s) {
    const int op = rnd(10);
    if (op < 4) {  // emplace: computeIfAbsent
      const int64_t k = base + rnd(12);
      const int32_t off = rnd(1 << 20);
      const auto had = model.find(k);
      EpochEnt* e = m.emplace(k, off);
      if (had != model.end()) {
        REQUIRE(e->id == k && e->offset == had->second);  // the existing entry, offset unchanged
        ++kept;
      } else {
        REQUIRE(e->id == k && e->offset == off && !e->shared);
        model[k] = off;
      }
    } else if (op < 6) {  // erase_below (checkpoint completion); base + 12 empties the map
      const int64_t k = base + rnd(13);
      m.erase_below(k);
      model.erase(model.begin(), model.lower_bound(k));
      for (Held& h : held)
        if (h.id < k) h.live = false;
      if (spilled && model.empty()) {
        ++emptied_after_spill;
        spilled = false;
      }
    } else if (op < 8) {  // rebase: the entries and the live shared objects move, stale ones stay
      const int32_t move = rnd(4096) - 1024;
      m.rebase(move);
      for (auto& kv : model) kv.second -= move;
      for (Held& h : held) {
        if (h.live) h.want -= move;
        else ++stale_checked;
      }
    } else if (!model.empty()) {  // ref: a consumer refers to an epoch
      auto it = model.begin();
      std::advance(it, rnd(int(model.size())));
      EpochEnt* e = m.find(it->first);
      REQUIRE(e != m.end());
      std::shared_ptr<EpochStart> p = EpochMap::ref(*e);
      REQUIRE(p && p == e->shared && p->id == it->first && p->offset == it->second);
      if (held.size() >= 24) held.erase(held.begin() + rnd(int(held.size())));
      held.push_back(Held{p, it->first, it->second, true});
    }
    REQUIRE(m.find(base - 1) == m.end() && m.find(base + 12) == m.end());
    if (model.size() >= 3) spilled = true;
    seen[std::min<size_t>(model.size(), 4)] = true;
    check_epochs(m, model, held);
  }
  for (bool b : seen) REQUIRE(b);
  REQUIRE(emptied_after_spill > 0 && kept > 0 && stale_checked > 0);
  // a reference outlives the map itself
  m.erase_below(base + 12);
  model.clear();
  for (Held& h : held) h.live = false;
  check_epochs(m, model, held);
}

// ---------------------------------------------------------------- SegList
static void check_segs(const SegList& l, const std::vector<uint32_t>& model) {
  REQUIRE(l.size() == model.size() && l.empty() == model.empty());
  REQUIRE(size_t(l.end() - l.begin()) == model.size());
  for (size_t i = 0; i < model.size(); ++i) REQUIRE(l[i] == model[i] && l.begin()[i] == model[i]);
}

struct SegPair {
  SegList l;
  std::vector<uint32_t> model;
  uint32_t next = 7;
  void push(size_t n) {
    for (size_t i = 0; i < n; ++i) {
      l.push_back(next);
      model.push_back(next);
      next = next * 2654435761u + 1;
      check_segs(l, model);
    }
  }
  void drop(size_t k) {
    l.erase_front(k);
    model.erase(model.begin(), model.begin() + long(k));
    check_segs(l, model);
  }
};

static void test_seg_list(uint32_t seed, int steps) {
  // the inline limit (6) from both sides: each erase_front followed by further push_backs
  for (size_t grow : {size_t(7), size_t(9), size_t(20)})
    for (size_t left : {size_t(6), size_t(5), size_t(1), size_t(0)}) {
      SegPair p;
      p.push(6);
      p.drop(0);
      p.push(grow - 6);  // 6 -> 7: the spill
      p.drop(0);
      p.drop(grow - left);  // a spilled list back to exactly 6, below 6, to 0
      p.push(8);            // and over the limit again
      p.drop(p.model.size());  // k = size
      p.push(3);
    }
  {
    SegPair p;  // inline only
    p.drop(0);
    p.push(6);
    p.drop(2);
    p.push(2);
    p.drop(6);
    p.push(1);
  }
  std::mt19937 rng(seed);
  SegPair p;
  for (int s = 0; s < steps; ++s) {
    if (rng() % 3) p.push(1 + rng() % 3);
    else p.drop(rng() % 4 == 0 ? (rng() % 2 ? p.model.size() : 0) : rng() % (p.model.size() + 1));
  }
}

// ---------------------------------------------------------------- EpochAlloc
// Blocks allocated on one thread are freed on another, which recycles some of them and then
// exits: its free list goes with it (no leak), and nothing is used after that.
static void test_epoch_alloc() {
  std::vector<std::shared_ptr<EpochStart>> made;
  std::thread a([&] {
    for (int i = 0; i < 1000; ++i)
      made.push_back(std::allocate_shared<EpochStart>(EpochAlloc<EpochStart>(), EpochStart{i, i * 3}));
  });
  a.join();
  std::shared_ptr<EpochStart> survivor;
  std::thread b([&] {
    for (int i = 0; i < 1000; ++i) REQUIRE(made[size_t(i)]->id == i && made[size_t(i)]->offset == i * 3);
    made.clear();  // freed here: the blocks join this thread's free list
    std::vector<std::shared_ptr<EpochStart>> again;
    for (int i = 0; i < 400; ++i)  // recycled
      again.push_back(std::allocate_shared<EpochStart>(EpochAlloc<EpochStart>(), EpochStart{-i, i}));
    for (int i = 0; i < 400; ++i) REQUIRE(again[size_t(i)]->id == -i && again[size_t(i)]->offset == i);
    survivor = again[7];  // one block outlives the thread that recycled it
  });
  b.join();
  REQUIRE(survivor->id == -7 && survivor->offset == 7);
  survivor.reset();  // freed on the main thread
  // through the map, as the engine does: an epoch referred to on one thread, dropped on another
  EpochMap m;
  std::shared_ptr<EpochStart> ref;
  std::thread c([&] { ref = EpochMap::ref(*m.emplace(5, 50)); });
  c.join();
  std::thread d([&] {
    m.emplace(6, 60);
    m.rebase(10);
    m.erase_below(6);
  });
  d.join();
  REQUIRE(ref->id == 5 && ref->offset == 40 && m.size() == 1 && m.begin()->offset == 50);
}

// ---------------------------------------------------------------- EngineLock
static void test_engine_lock() {
  EngineLock L;
  std::atomic<int> started{0}, got{0};
  REQUIRE(!L.owned());
  L.lock();
  REQUIRE(L.owned());
  {
    XGuard again(L);  // re-entrant: depth 2
    REQUIRE(L.owned() && L.depth == 2);
  }
  L.lock();
  std::thread t([&] {
    REQUIRE(!L.owned());
    started.store(1);
    std::lock_guard<std::mutex> g(L.stripe[5].m);  // a per-log call: only its stripe
    REQUIRE(!L.owned());
    got.store(1);
  });
  while (!started.load()) std::this_thread::yield();
  for (int i = 0; i < 2000; ++i) std::this_thread::yield();
  REQUIRE(got.load() == 0);  // excluded while the lock is held
  L.unlock();                // depth 2 -> 1: still held
  REQUIRE(L.owned() && L.depth == 1);
  for (int i = 0; i < 2000; ++i) std::this_thread::yield();
  REQUIRE(got.load() == 0);
  L.unlock();
  REQUIRE(!L.owned());
  t.join();
  REQUIRE(got.load() == 1);
  // and the other way round: the exclusive lock waits for a stripe's holder
  std::atomic<int> excl{0};
  std::unique_lock<std::mutex> stripe(L.stripe[63].m);
  started.store(0);
  std::thread u([&] {
    started.store(1);
    XGuard g(L);
    excl.store(1);
  });
  while (!started.load()) std::this_thread::yield();
  for (int i = 0; i < 2000; ++i) std::this_thread::yield();
  REQUIRE(excl.load() == 0);
  stripe.unlock();
  u.join();
  REQUIRE(excl.load() == 1 && !L.owned());
}

// ---------------------------------------------------------------- WorkPool
static void test_work_pool(unsigned n, int calls) {
  std::atomic<uint64_t> sum{0};
  uint64_t want = 0;
  {
    WorkPool pool(n);
    REQUIRE(pool.size() == n);
    for (int i = 0; i < calls; ++i) {
      // most calls follow at once (the workers still spin); some after a gap longer than their
      // 50 us spin (they sleep on the condition variable)
      if (i % 256 == 255) std::this_thread::sleep_for(std::chrono::microseconds(400));
      pool.run([&](unsigned k, unsigned parts) {
        REQUIRE(parts == n && k < parts);
        sum.fetch_add(uint64_t(i + 1) * (k + 1), std::memory_order_relaxed);
      });
      want += uint64_t(i + 1) * (uint64_t(n) * (n + 1) / 2);
      REQUIRE(sum.load() == want);  // run() returns once every part has run
    }
  }  // destroyed right after a run
  REQUIRE(sum.load() == want);
  for (int r = 0; r < 20; ++r) {
    WorkPool pool(n);
    if (r % 2) pool.run([&](unsigned, unsigned) { sum.fetch_add(1, std::memory_order_relaxed); });
  }  // (and without any run)
  REQUIRE(sum.load() == want + 10 * n);
}

// ---------------------------------------------------------------- for_each_chunk, chunk_count
// Against a byte-by-byte model: the bytes of [at, at + n) taken one at a time, a byte opening a
// new chunk when it is the first one or lies at a multiple of C.  (For one `at` the model of n
// is the model of n - 1 and one more byte.)
static void test_chunks(uint32_t C) {
  struct Chunk {
    uint32_t start, len;
  };
  for (uint32_t at = 0; at <= 2 * C + 1; ++at) {
    std::vector<Chunk> model;
    for (uint32_t n = 0; n <= 3 * C + 1; ++n) {
      if (n) {
        const uint32_t b = at + n - 1;
        if (model.empty() || b % C == 0) model.push_back(Chunk{b, 1});
        else ++model.back().len;
      }
      size_t k = 0;
      uint32_t next = at;
      bool last_seen = false;
      for_each_chunk(at, n, C, [&](uint32_t si, uint32_t so, uint32_t take, bool more) {
        REQUIRE(k < model.size() && !last_seen);
        REQUIRE(take > 0 && so < C && so + take <= C);  // inside one segment
        REQUIRE(si * C + so == next && next == model[k].start && take == model[k].len);  // in order, no gap or overlap
        REQUIRE(more == (k + 1 != model.size()));
        last_seen = !more;
        next += take;
        ++k;
      });
      REQUIRE(k == model.size() && next == at + n);
      REQUIRE((n == 0) == (k == 0) && (k == 0 || last_seen));
      REQUIRE(chunk_count(at, n, C) == k && k <= n / C + 2);
    }
  }
}

int main() {
  for (uint32_t C : {16u, 64u, 256u}) test_chunks(C);
  for (uint32_t seed = 1; seed <= 4; ++seed) test_epoch_map(seed, 6000);
  for (uint32_t seed = 1; seed <= 4; ++seed) test_seg_list(seed, 4000);
  test_epoch_alloc();
  test_engine_lock();
  test_work_pool(1, 3000);
  test_work_pool(4, 3000);
  printf("engine_host: ok\n");
  return 0;
}
