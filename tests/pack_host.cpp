// Stand-alone check of the CPU pack and unpack of typed columns (clonos_amd/csrc/pack.h) against
// a naive reference packer kept here, which sets the payload one bit at a time with 128-bit
// arithmetic and shares nothing with the header: every width 0..64 for the DELTA stream, every
// width the type allows for the FOR streams, block lengths 0, 1, 2, 1023, 1024, 1025 and 2049,
// constant blocks, INT64_MIN beside INT64_MAX, zero padding, the unpack of every sub-range edge,
// sizes only, the capacity failures over filled outputs, and every malformed-input rejection.  Built
// with g++ (no HIP), plainly and with -fsanitize=address,undefined; every array is allocated at
// its exact size so that a read or write past a stated length is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../clonos_amd/csrc/pack.h"

namespace {

uint64_t g_checks = 0;
#define REQUIRE(x)                                                     \
  do {                                                                 \
    ++g_checks;                                                        \
    if (!(x)) {                                                        \
      fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

typedef __int128 i128;

struct Cols {
  std::vector<uint8_t> tag;
  std::vector<int8_t> order;
  std::vector<int64_t> timestamp;
  std::vector<int32_t> rng, buffer_built;
  clg_columns c() const {
    clg_columns x{};
    x.tag = const_cast<uint8_t*>(tag.data()), x.order = const_cast<int8_t*>(order.data());
    x.timestamp = const_cast<int64_t*>(timestamp.data()), x.rng = const_cast<int32_t*>(rng.data());
    x.buffer_built = const_cast<int32_t*>(buffer_built.data());
    x.n_rec = tag.size(), x.n_class[0] = order.size(), x.n_class[1] = timestamp.size();
    x.n_class[2] = rng.size(), x.n_class[3] = buffer_built.size();
    return x;
  }
  std::vector<int64_t> wide(uint32_t s) const {  // stream s extended to 64 bits
    std::vector<int64_t> v;
    if (s == 0) for (uint8_t x : tag) v.push_back(x);
    if (s == 1) for (int8_t x : order) v.push_back(x);
    if (s == 2) v = timestamp;
    if (s == 3) for (int32_t x : rng) v.push_back(x);
    if (s == 4) for (int32_t x : buffer_built) v.push_back(x);
    return v;
  }
};

struct Ref {
  std::vector<clg_pack_block> desc;
  std::vector<uint8_t> bits;
  uint64_t blk_base[6];
};

// The reference: residuals in 128-bit arithmetic reduced modulo 2^64, the payload bit by bit.
Ref reference(const Cols& cols) {
  Ref r;
  r.blk_base[0] = 0;
  for (uint32_t s = 0; s < 5; ++s) {
    const std::vector<int64_t> v = cols.wide(s);
    const bool delta = s == 2;
    for (size_t i0 = 0; i0 < v.size(); i0 += 1024) {
      const size_t m = v.size() - i0 < 1024 ? v.size() - i0 : 1024;
      std::vector<int64_t> res;
      for (size_t i = delta ? 1 : 0; i < m; ++i) {
        i128 x = v[i0 + i];
        if (delta) x -= i128(v[i0 + i - 1]);
        res.push_back(int64_t(uint64_t(x)));  // modulo 2^64, read back as signed
      }
      clg_pack_block d{};
      d.count = uint32_t(m);
      d.first = delta ? v[i0] : 0;
      d.pos = r.bits.size();
      if (!res.empty()) {
        int64_t lo = res[0], hi = res[0];
        for (int64_t x : res) lo = x < lo ? x : lo, hi = x > hi ? x : hi;
        const i128 range = i128(hi) - i128(lo);
        uint32_t width = 0;
        while (width < 64 && (range >> width) != 0) ++width;
        d.ref = lo, d.width = width;
        const size_t nbit = res.size() * width, nbyte = 16 * ((nbit + 127) / 128);
        r.bits.resize(r.bits.size() + nbyte, 0);
        for (size_t i = 0; i < res.size(); ++i) {
          const i128 p = i128(res[i]) - i128(lo);
          for (uint32_t b = 0; b < width; ++b)
            if ((p >> b) & 1) r.bits[d.pos + (i * width + b) / 8] |= uint8_t(1u << ((i * width + b) % 8));
        }
      }
      r.desc.push_back(d);
    }
    r.blk_base[s + 1] = r.desc.size();
  }
  return r;
}

constexpr uint8_t kFill = 0xA5;

// Exactly sized outputs, each its own allocation (the sanitizer sees an overrun), filled with
// kFill so that a call that must write nothing can be held to it.
struct Out {
  std::vector<clg_pack_block> desc;
  std::vector<uint8_t> bits;
  clg_packed p{};
  Out(size_t nb, size_t nbits) : desc(nb), bits(nbits, kFill) {
    if (nb) memset(desc.data(), kFill, nb * sizeof(clg_pack_block));
    p.desc = nb ? desc.data() : nullptr, p.bits = nbits ? bits.data() : nullptr;
    p.cap_desc = nb, p.cap_bits = nbits;
  }
  bool untouched() const {
    for (size_t i = 0; i < desc.size() * sizeof(clg_pack_block); ++i)
      if (reinterpret_cast<const uint8_t*>(desc.data())[i] != kFill) return false;
    for (uint8_t b : bits)
      if (b != kFill) return false;
    return true;
  }
};

template <class T>
void unpack_check(const clg_packed& p, uint32_t s, const std::vector<T>& want) {
  const uint64_t n = want.size();
  // the whole stream, then every edge: the first and last value of each block, ranges that end at
  // and straddle a block boundary, the empty range at every edge
  std::vector<std::pair<uint64_t, uint64_t>> ranges = {{0, n}, {n, 0}, {0, 0}};
  for (uint64_t b = 0; b * 1024 < n; ++b) {
    const uint64_t lo = b * 1024, hi = lo + 1024 < n ? lo + 1024 : n;
    ranges.push_back({lo, 1}), ranges.push_back({hi - 1, 1}), ranges.push_back({lo, hi - lo});
    if (hi < n) ranges.push_back({hi - 1, 2}), ranges.push_back({hi - 3 < lo ? lo : hi - 3, (n - hi < 5 ? n - hi : 5) + (hi - (hi - 3 < lo ? lo : hi - 3))});
    if (hi - lo > 2) ranges.push_back({lo + 1, hi - lo - 2});
  }
  for (auto [first, count] : ranges) {
    std::vector<T> got(count);  // exactly sized
    REQUIRE(clg::pack_unpack_host(&p, s, first, count, count ? got.data() : nullptr) == CLG_OK);
    for (uint64_t i = 0; i < count; ++i) REQUIRE(got[i] == want[first + i]);
  }
  T one;
  REQUIRE(clg::pack_unpack_host(&p, s, n, 1, &one) == CLG_E_INVALID_ARG);
  REQUIRE(clg::pack_unpack_host(&p, s, n + 1, 0, &one) == CLG_E_INVALID_ARG);
  REQUIRE(clg::pack_unpack_host(&p, s, 1, ~0ull, &one) == CLG_E_INVALID_ARG);
}

// Pack `cols` and hold the result against the reference, byte for byte; then the round trip.
clg_packed check(const Cols& cols, Out** keep = nullptr) {
  const Ref want = reference(cols);
  const clg_columns in = cols.c();
  clg_packed sizes{};
  REQUIRE(clg::pack_build_host(&in, &sizes) == CLG_OK);  // sizes only
  REQUIRE(sizes.n_bits == want.bits.size());
  for (int s = 0; s <= 5; ++s) REQUIRE(sizes.blk_base[s] == want.blk_base[s]);
  REQUIRE(sizes.n_val[0] == cols.tag.size() && sizes.n_val[2] == cols.timestamp.size());
  REQUIRE(want.bits.size() % 16 == 0);

  Out* o = new Out(want.desc.size(), want.bits.size());
  REQUIRE(clg::pack_build_host(&in, &o->p) == CLG_OK);
  REQUIRE(o->p.n_bits == want.bits.size());
  for (size_t b = 0; b < want.desc.size(); ++b) {
    const clg_pack_block &g = o->desc[b], &w = want.desc[b];
    REQUIRE(g.ref == w.ref && g.first == w.first && g.pos == w.pos && g.width == w.width && g.count == w.count);
    REQUIRE(g.pos % 16 == 0);
  }
  REQUIRE(o->bits == want.bits);  // (the padding bits included: the reference leaves them zero)

  unpack_check(o->p, 0, cols.tag);
  unpack_check(o->p, 1, cols.order);
  unpack_check(o->p, 2, cols.timestamp);
  unpack_check(o->p, 3, cols.rng);
  unpack_check(o->p, 4, cols.buffer_built);

  // a capacity one short, each array in turn: the sizes are filled and nothing is written
  if (!want.desc.empty()) {
    Out s(want.desc.size() - 1, want.bits.size());
    REQUIRE(clg::pack_build_host(&in, &s.p) == CLG_E_CAPACITY);
    REQUIRE(s.p.n_bits == want.bits.size() && s.p.blk_base[5] == want.desc.size() && s.untouched());
  }
  if (!want.bits.empty()) {
    Out s(want.desc.size(), want.bits.size() - 1);
    REQUIRE(clg::pack_build_host(&in, &s.p) == CLG_E_CAPACITY);
    REQUIRE(s.p.n_bits == want.bits.size() && s.untouched());
  }
  const clg_packed p = o->p;
  if (keep) *keep = o; else delete o;
  return p;
}

// n values whose residuals span exactly `width` bits from the signed minimum `lo`.
std::vector<uint64_t> residuals(std::mt19937_64& r, uint32_t width, size_t n, int64_t lo) {
  std::vector<uint64_t> v(n);
  const uint64_t span = width == 64 ? ~0ull : (1ull << width) - 1;
  for (uint64_t& x : v) x = uint64_t(lo) + (span == ~0ull ? r() : r() % (span + 1));
  if (n >= 2 && width) {  // both ends present, at distinct places
    const size_t a = r() % n, b = (a + 1 + r() % (n - 1)) % n;
    v[a] = uint64_t(lo), v[b] = uint64_t(lo) + span;
  }
  return v;
}

uint32_t width_of(const clg_packed& p, uint32_t s, uint64_t b = 0) { return p.desc[p.blk_base[s] + b].width; }

void widths() {
  std::mt19937_64 r(0xFACADE);
  const size_t lens[] = {3, 64, 1023, 1024};
  for (uint32_t w = 0; w <= 64; ++w)
    for (size_t n : lens) {
      Cols c;
      // DELTA: n + 1 values, n residuals of width w from a signed minimum that keeps lo + span in int64
      const uint64_t span = w == 64 ? ~0ull : (1ull << w) - 1;
      const int64_t lo = w == 64 ? INT64_MIN : int64_t(r() % (uint64_t(INT64_MAX) - span / 2 + 1)) - int64_t(span / 2) - (w == 63 ? INT64_MAX / 2 : 0);
      const int64_t lo_ok = (i128(lo) + i128(span) > i128(INT64_MAX)) ? int64_t(i128(INT64_MAX) - i128(span)) : lo;
      uint64_t x = r();
      c.timestamp.push_back(int64_t(x));
      if (n < 1024)
        for (uint64_t d : residuals(r, w, n, lo_ok)) c.timestamp.push_back(int64_t(x += d));
      else
        for (uint64_t d : residuals(r, w, 1023, lo_ok)) c.timestamp.push_back(int64_t(x += d));
      // FOR: every width the type allows
      if (w <= 3) for (uint64_t v : residuals(r, w, n, int64_t(r() % (8 - ((1u << w) - 1))))) c.tag.push_back(uint8_t(v));
      if (w <= 8) for (uint64_t v : residuals(r, w, n, -128 + int64_t(r() % (256 - ((1u << w) - 1))))) c.order.push_back(int8_t(int64_t(v)));
      if (w <= 32) {
        const uint64_t sp = (1ull << w) - 1;
        for (uint64_t v : residuals(r, w, n, INT32_MIN + int64_t(r() % ((1ull << 32) - sp)))) c.rng.push_back(int32_t(int64_t(v)));
        for (uint64_t v : residuals(r, w, n, INT32_MAX - int64_t(sp))) c.buffer_built.push_back(int32_t(int64_t(v)));
      }
      Out* o = nullptr;
      const clg_packed p = check(c, &o);
      REQUIRE(width_of(p, 2) == w);
      if (w <= 3) REQUIRE(width_of(p, 0) == w);
      if (w <= 8) REQUIRE(width_of(p, 1) == w);
      if (w <= 32) REQUIRE(width_of(p, 3) == w && width_of(p, 4) == w);
      delete o;
    }
}

void lengths() {
  std::mt19937_64 r(0xBEEF);
  const size_t lens[] = {0, 1, 2, 1023, 1024, 1025, 2049};
  for (size_t n : lens)
    for (int variant = 0; variant < 3; ++variant) {
      Cols c;
      int64_t t = 1700000000000ll;
      for (size_t i = 0; i < n; ++i) {
        c.tag.push_back(variant == 1 ? 7 : uint8_t(r() % 8));            // variant 1: constant blocks (width 0)
        c.order.push_back(variant == 1 ? -3 : int8_t(r() % 4));
        c.timestamp.push_back(variant == 1 ? t += 5 : t += int64_t(r() % 6));  // a constant step: width 0
        c.rng.push_back(variant == 1 ? INT32_MIN : int32_t(r()));
        c.buffer_built.push_back(variant == 2 ? int32_t(r() % 65536) : 4096);
      }
      if (variant == 2) c.order.clear(), c.rng.clear();  // streams of different lengths, some empty
      Out* o = nullptr;
      const clg_packed p = check(c, &o);
      if (variant == 1 && n) {
        REQUIRE(p.n_bits == 0);
        for (uint64_t b = 0; b < p.blk_base[5]; ++b) REQUIRE(p.desc[b].width == 0);
      }
      delete o;
    }
}

void extremes() {
  Cols c;
  const int64_t pat[] = {INT64_MIN, INT64_MAX, INT64_MIN, 0, INT64_MAX, INT64_MAX, INT64_MIN, -1, 1};
  for (int k = 0; k < 300; ++k)
    for (int64_t v : pat) c.timestamp.push_back(v);
  c.rng = {INT32_MIN, INT32_MAX, INT32_MIN, -1, 0, 1, INT32_MAX};
  c.order = {-128, 127, -128, 0};
  c.tag = {0, 255, 7, 0};  // (the pack takes any byte; the columns' own rules are the columnize's)
  Out* o = nullptr;
  const clg_packed p = check(c, &o);
  REQUIRE(width_of(p, 3) == 32 && width_of(p, 1) == 8 && width_of(p, 0) == 8);
  delete o;
}

// Every rejection of clg_unpack_columns_host: the bytes may come from another process.
void malformed() {
  std::mt19937_64 r(0xBAD);
  Cols c;
  int64_t t = 0;
  for (int i = 0; i < 2500; ++i) c.timestamp.push_back(t += int64_t(r() % 1000)), c.rng.push_back(int32_t(r() % 100000));
  for (int i = 0; i < 1500; ++i) c.tag.push_back(uint8_t(r() % 8)), c.order.push_back(int8_t(r() % 4));
  Out* o = nullptr;
  const clg_packed good = check(c, &o);
  std::vector<int64_t> out64(2500);
  std::vector<int32_t> out32(2500);
  std::vector<uint8_t> out8(1500);
  const auto ts = [&](const clg_packed& p) { return clg::pack_unpack_host(&p, 2, 0, 2500, out64.data()); };
  REQUIRE(ts(good) == CLG_OK);
  const auto bad = [&](const clg_packed& p) { REQUIRE(ts(p) == CLG_E_INVALID_ARG); };
  const uint64_t b0 = good.blk_base[2];
  const clg_pack_block saved[3] = {o->desc[b0], o->desc[b0 + 1], o->desc[b0 + 2]};
  const auto restore = [&] { o->desc[b0] = saved[0], o->desc[b0 + 1] = saved[1], o->desc[b0 + 2] = saved[2]; };

  o->desc[b0 + 1].width = 65; bad(good); restore();
  o->desc[b0 + 1].width = 0xFFFFFFFFu; bad(good); restore();
  o->desc[b0].count = 0; bad(good); restore();
  o->desc[b0].count = 1025; bad(good); restore();
  o->desc[b0].count = 1023; bad(good); restore();      // not the last block: 1024
  o->desc[b0 + 2].count = 453; bad(good); restore();    // the last block: 2500 - 2048
  o->desc[b0 + 2].count = 1024; bad(good); restore();
  o->desc[b0 + 2].pos = good.n_bits; bad(good); restore();          // pos + size > n_bits
  o->desc[b0 + 2].pos = ~0ull - 15; bad(good); restore();           // ... wrapping
  o->desc[b0 + 1].width = 64; bad(good); restore();                 // its size passes n_bits
  {
    clg_packed p = good;
    p.n_bits = 16; bad(p);  // (the blocks read lie past it)
    p = good, p.n_bits = p.cap_bits + 16; bad(p);
    p = good, p.blk_base[3] += 1; bad(p);
    p = good, p.blk_base[2] = p.blk_base[3] + 1; bad(p);
    p = good, p.cap_desc = p.blk_base[3] - 1; bad(p);
    p = good, p.n_val[2] = 2500 + 1024; bad(p);
    p = good, p.desc = nullptr; bad(p);
    p = good, p.bits = nullptr; bad(p);
    REQUIRE(clg::pack_unpack_host(&good, 5, 0, 0, out64.data()) == CLG_E_INVALID_ARG);
    REQUIRE(clg::pack_unpack_host(nullptr, 0, 0, 0, out64.data()) == CLG_E_INVALID_ARG);
    REQUIRE(clg::pack_unpack_host(&good, 2, 0, 1, nullptr) == CLG_E_INVALID_ARG);
  }
  // values outside the stream's type: an i32 block whose reference or width reaches past int32, a
  // tag above 255 or below 0, a channel outside a Java byte
  const auto bad_value = [&](uint32_t s, void* out, uint64_t n, auto&& poke) {
    const uint64_t b = good.blk_base[s];
    const clg_pack_block keep = o->desc[b];
    poke(o->desc[b]);
    REQUIRE(clg::pack_unpack_host(&good, s, 0, n, out) == CLG_E_INVALID_ARG);
    o->desc[b] = keep;
    REQUIRE(clg::pack_unpack_host(&good, s, 0, n, out) == CLG_OK);
  };
  bad_value(3, out32.data(), 2500, [](clg_pack_block& d) { d.ref = int64_t(INT32_MAX) - 5; });
  bad_value(3, out32.data(), 2500, [](clg_pack_block& d) { d.ref = int64_t(INT32_MIN) - 1; });
  bad_value(0, out8.data(), 1500, [](clg_pack_block& d) { d.ref = 250; });
  bad_value(0, out8.data(), 1500, [](clg_pack_block& d) { d.ref = -1; });
  bad_value(1, out8.data(), 1500, [](clg_pack_block& d) { d.ref = 126; });
  bad_value(1, out8.data(), 1500, [](clg_pack_block& d) { d.ref = -131; });
  delete o;

  // the pack's own argument checks
  clg_packed p{};
  clg_columns in = c.c();
  REQUIRE(clg::pack_build_host(nullptr, &p) == CLG_E_INVALID_ARG && clg::pack_build_host(&in, nullptr) == CLG_E_INVALID_ARG);
  in.rng = nullptr;
  REQUIRE(clg::pack_build_host(&in, &p) == CLG_E_INVALID_ARG);
}

}  // namespace

int main() {
  widths();
  lengths();
  extremes();
  malformed();
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
