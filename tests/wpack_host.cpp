// Stand-alone check of the CPU pack and unpack of wide rows (clonos_amd/csrc/pack_wide.h) against a
// naive reference kept here, which partitions the rows with plain loops, keeps its own copy of the
// scheme table, sets the payload one bit at a time with 128-bit arithmetic and shares nothing with
// the header: row counts 0, 1, 2, 1023, 1024, 1025 and 2049, each kind absent, alone and mixed,
// every width 0..64 on the i64 fields, 0..32 on the 32-bit fields and 0..8 on SUB, INT64_MIN beside
// INT64_MAX, the round trip, sizes only, the capacity failures over filled outputs, the lowest of
// several bad rows, and every rejection of the unpack with its report and its output untouched.
// Built with g++ (no HIP), plainly and with -fsanitize=address,undefined; every array is allocated
// at its exact size so that a read or write past a stated length is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../clonos_amd/csrc/pack_wide.h"

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

struct Rows {
  std::vector<uint8_t> tag;
  std::vector<uint32_t> idx;
  std::vector<int32_t> rc;
  std::vector<int64_t> v1;
  std::vector<uint32_t> off, len;
  std::vector<uint8_t> sub;
  std::vector<int64_t> v0;
  // a row of `kind` behind a fresh record of its tag (narrow records between the wide ones)
  void add(uint32_t kind, int32_t rc_, int64_t v1_, uint32_t off_, uint32_t len_, uint8_t sub_, int64_t v0_, uint32_t narrow = 0) {
    for (uint32_t i = 0; i < narrow; ++i) tag.push_back(uint8_t(i % 3));
    idx.push_back(uint32_t(tag.size()));
    tag.push_back(uint8_t(3 + kind));
    rc.push_back(rc_), v1.push_back(v1_), off.push_back(off_), len.push_back(len_), sub.push_back(sub_), v0.push_back(v0_);
  }
  clg_columns c() const {
    clg_columns x{};
    x.tag = const_cast<uint8_t*>(tag.data()), x.w_idx = const_cast<uint32_t*>(idx.data());
    x.w_rc = const_cast<int32_t*>(rc.data()), x.w_v1 = const_cast<int64_t*>(v1.data());
    x.w_var_off = const_cast<uint32_t*>(off.data()), x.w_var_len = const_cast<uint32_t*>(len.data());
    x.w_sub = const_cast<uint8_t*>(sub.data()), x.w_v0 = const_cast<int64_t*>(v0.data());
    x.n_rec = tag.size(), x.n_class[4] = idx.size();
    return x;
  }
};

struct Ref {
  std::vector<clg_pack_block> desc;
  std::vector<uint8_t> bits;
  uint64_t n_val[26], blk_base[27];
};

// The reference's own scheme table: 1 = DELTA.  Stream 0 KIND, 1 IDX, then RC V1 VAR_OFF VAR_LEN
// SUB V0 per kind.
const int kDelta[26] = {0, 1, /*kind 0*/ 0, 1, 1, 0, 0, 0, /*1*/ 0, 1, 1, 0, 0, 1, /*2*/ 0, 1, 1, 0, 0, 1, /*3*/ 0, 1, 1, 0, 0, 1};

Ref reference(const Rows& r) {
  std::vector<int64_t> v[26];
  for (size_t k = 0; k < r.idx.size(); ++k) {
    const int kind = int(r.tag[r.idx[k]]) - 3;
    v[0].push_back(kind), v[1].push_back(int64_t(r.idx[k]));
    v[2 + 6 * kind + 0].push_back(r.rc[k]), v[2 + 6 * kind + 1].push_back(r.v1[k]);
    v[2 + 6 * kind + 2].push_back(int64_t(r.off[k])), v[2 + 6 * kind + 3].push_back(int64_t(r.len[k]));
    v[2 + 6 * kind + 4].push_back(r.sub[k]), v[2 + 6 * kind + 5].push_back(r.v0[k]);
  }
  Ref out;
  out.blk_base[0] = 0;
  for (uint32_t s = 0; s < 26; ++s) {
    const bool delta = kDelta[s] != 0;
    out.n_val[s] = v[s].size();
    for (size_t i0 = 0; i0 < v[s].size(); i0 += 1024) {
      const size_t m = v[s].size() - i0 < 1024 ? v[s].size() - i0 : 1024;
      std::vector<int64_t> res;
      for (size_t i = delta ? 1 : 0; i < m; ++i) {
        i128 x = v[s][i0 + i];
        if (delta) x -= i128(v[s][i0 + i - 1]);
        res.push_back(int64_t(uint64_t(x)));  // modulo 2^64, read back as signed
      }
      clg_pack_block d{};
      d.count = uint32_t(m);
      d.first = delta ? v[s][i0] : 0;
      d.pos = out.bits.size();
      if (!res.empty()) {
        int64_t lo = res[0], hi = res[0];
        for (int64_t x : res) lo = x < lo ? x : lo, hi = x > hi ? x : hi;
        const i128 range = i128(hi) - i128(lo);
        uint32_t width = 0;
        while (width < 64 && (range >> width) != 0) ++width;
        d.ref = lo, d.width = width;
        const size_t nbit = res.size() * width, nbyte = 16 * ((nbit + 127) / 128);
        out.bits.resize(out.bits.size() + nbyte, 0);
        for (size_t i = 0; i < res.size(); ++i) {
          const i128 p = i128(res[i]) - i128(lo);
          for (uint32_t b = 0; b < width; ++b)
            if ((p >> b) & 1) out.bits[d.pos + (i * width + b) / 8] |= uint8_t(1u << ((i * width + b) % 8));
        }
      }
      out.desc.push_back(d);
    }
    out.blk_base[s + 1] = out.desc.size();
  }
  return out;
}

constexpr uint8_t kFill = 0xA5;

// Exactly sized outputs, each its own allocation, filled with kFill.
struct Out {
  std::vector<clg_pack_block> desc;
  std::vector<uint8_t> bits;
  clg_packed_wide p{};
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

// Exactly sized arrays for the unpack, filled with kFill.
struct Back {
  std::vector<uint32_t> idx, off, len;
  std::vector<int32_t> rc;
  std::vector<int64_t> v1, v0;
  std::vector<uint8_t> sub;
  clg_columns c{};
  explicit Back(size_t n) : idx(n, 0xA5A5A5A5u), off(n, 0xA5A5A5A5u), len(n, 0xA5A5A5A5u), rc(n, int32_t(0xA5A5A5A5u)),
                            v1(n, int64_t(0xA5A5A5A5A5A5A5A5ull)), v0(n, int64_t(0xA5A5A5A5A5A5A5A5ull)), sub(n, kFill) {
    c.w_idx = idx.data(), c.w_rc = rc.data(), c.w_v1 = v1.data(), c.w_var_off = off.data(), c.w_var_len = len.data();
    c.w_sub = sub.data(), c.w_v0 = v0.data(), c.cap_wide = n;
    c.n_class[4] = 0xDEAD;
  }
  bool untouched() const {
    for (size_t i = 0; i < idx.size(); ++i)
      if (idx[i] != 0xA5A5A5A5u || off[i] != 0xA5A5A5A5u || len[i] != 0xA5A5A5A5u || rc[i] != int32_t(0xA5A5A5A5u) ||
          v1[i] != int64_t(0xA5A5A5A5A5A5A5A5ull) || v0[i] != int64_t(0xA5A5A5A5A5A5A5A5ull) || sub[i] != kFill)
        return false;
    return true;
  }
  bool equals(const Rows& r) const {
    return idx == r.idx && rc == r.rc && v1 == r.v1 && off == r.off && len == r.len && sub == r.sub && v0 == r.v0;
  }
};

// Pack `rows` and hold the result against the reference, byte for byte; then the round trip and the
// capacity failures.
Out* check(const Rows& rows) {
  const Ref want = reference(rows);
  const clg_columns in = rows.c();
  clg_packed_wide sizes{};
  REQUIRE(clg::wpack_build_host(&in, &sizes) == CLG_OK);  // sizes only
  REQUIRE(sizes.n_bits == want.bits.size() && sizes.bad_row == ~0ull);
  for (int s = 0; s <= 26; ++s) REQUIRE(sizes.blk_base[s] == want.blk_base[s]);
  for (int s = 0; s < 26; ++s) REQUIRE(sizes.n_val[s] == want.n_val[s]);
  REQUIRE(want.bits.size() % 16 == 0);

  Out* o = new Out(want.desc.size(), want.bits.size());
  REQUIRE(clg::wpack_build_host(&in, &o->p) == CLG_OK);
  REQUIRE(o->p.n_bits == want.bits.size());
  for (size_t b = 0; b < want.desc.size(); ++b) {
    const clg_pack_block &g = o->desc[b], &w = want.desc[b];
    REQUIRE(g.ref == w.ref && g.first == w.first && g.pos == w.pos && g.width == w.width && g.count == w.count);
    REQUIRE(g.pos % 16 == 0);
  }
  REQUIRE(o->bits == want.bits);  // (the padding bits included: the reference leaves them zero)

  // the round trip: sizes only, one row short, then the arrays
  clg_columns so{};
  so.n_class[4] = 0xDEAD;
  clg_unpack_bad bad;
  REQUIRE(clg::wpack_unpack_host(&o->p, &so, &bad) == CLG_OK && so.n_class[4] == rows.idx.size() && bad.what == CLG_UNPACK_BAD_NONE);
  if (rows.idx.size() > 1) {  // (no array at all is the sizes-only call)
    Back s(rows.idx.size() - 1);
    REQUIRE(clg::wpack_unpack_host(&o->p, &s.c, &bad) == CLG_E_CAPACITY && s.c.n_class[4] == rows.idx.size() && s.untouched());
  }
  Back back(rows.idx.size());
  REQUIRE(clg::wpack_unpack_host(&o->p, &back.c, &bad) == CLG_OK);
  REQUIRE(back.c.n_class[4] == rows.idx.size() && back.equals(rows) && bad.what == CLG_UNPACK_BAD_NONE && bad.block == ~0ull);

  // a capacity one short, each array in turn: the sizes are filled and nothing is written
  if (!want.desc.empty()) {
    Out s(want.desc.size() - 1, want.bits.size());
    REQUIRE(clg::wpack_build_host(&in, &s.p) == CLG_E_CAPACITY);
    REQUIRE(s.p.n_bits == want.bits.size() && s.p.blk_base[26] == want.desc.size() && s.untouched());
  }
  if (!want.bits.empty()) {
    Out s(want.desc.size(), want.bits.size() - 1);
    REQUIRE(clg::wpack_build_host(&in, &s.p) == CLG_E_CAPACITY);
    REQUIRE(s.p.n_bits == want.bits.size() && s.untouched());
  }
  return o;
}

// n residuals that span exactly `width` bits from the signed minimum `lo`.
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

uint32_t width_of(const clg_packed_wide& p, uint32_t s, uint64_t b = 0) { return p.desc[p.blk_base[s] + b].width; }

// A believable mixed batch: kinds by `pick`, counters and clocks.
Rows mixed(std::mt19937_64& r, size_t n, int only_kind = -1, int without_kind = -1) {
  Rows rows;
  int64_t clock = 1700000000000ll, cp = 40;
  uint32_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t kind = only_kind >= 0 ? uint32_t(only_kind) : uint32_t(r() % 4);
    if (int(kind) == without_kind) kind = (kind + 1) % 4;
    off += 9 + uint32_t(r() % 40);
    clock += int64_t(r() % 50), ++cp;
    if (kind == 0) rows.add(0, int32_t(r() >> 33), 0, off, uint32_t(r() % 300), 0, int64_t(r() % 300), uint32_t(r() % 4));
    else if (kind == 1) rows.add(1, int32_t(r() >> 33), clock, off, uint32_t(r() % 64), uint8_t(r() % 3), clock - 7, uint32_t(r() % 4));
    else rows.add(kind, int32_t(r() >> 33), clock + 3, off, uint32_t(r() % 16), uint8_t(r() % 2), cp, uint32_t(r() % 4));
  }
  return rows;
}

void lengths() {
  std::mt19937_64 r(0xBEEF);
  const size_t lens[] = {0, 1, 2, 1023, 1024, 1025, 2049};
  for (size_t n : lens) {
    delete check(mixed(r, n));
    for (int t = 0; t < 4; ++t) {
      delete check(mixed(r, n, t));      // one kind only
      delete check(mixed(r, n, -1, t));  // one kind absent
    }
  }
  // a kind that uses no field: all zeros, a width-0 descriptor a block and no payload byte
  Rows z;
  for (int i = 0; i < 2049; ++i) z.add(3, 0, 0, 0, 0, 0, 0);
  Out* o = check(z);
  for (uint32_t f = 0; f < 6; ++f)
    for (uint64_t b = 0; b < 3; ++b) REQUIRE(width_of(o->p, 2 + 6 * 3 + f, b) == 0);
  REQUIRE(o->p.blk_base[26] == 3 + 3 + 6 * 3);
  delete o;
}

void widths() {
  std::mt19937_64 r(0xFACADE);
  const size_t lens[] = {3, 64, 1023, 1024};
  for (uint32_t w = 0; w <= 64; ++w)
    for (size_t n : lens)
      for (uint32_t kind = 0; kind < 4; ++kind) {
        const uint64_t span = w == 64 ? ~0ull : (1ull << w) - 1;
        const int64_t lo0 = w == 64 ? INT64_MIN : int64_t(r() % (uint64_t(INT64_MAX) - span / 2 + 1)) - int64_t(span / 2) - (w == 63 ? INT64_MAX / 2 : 0);
        const int64_t lo = (i128(lo0) + i128(span) > i128(INT64_MAX)) ? int64_t(i128(INT64_MAX) - i128(span)) : lo0;
        // DELTA fields: n values, n - 1 residuals of width w; FOR fields: n values of width w
        const size_t nr = n - 1;
        const std::vector<uint64_t> d1 = residuals(r, w, nr, lo), d0 = residuals(r, w, kind ? nr : n, lo);
        const uint32_t w32 = w < 32 ? w : 32, w8 = w < 8 ? w : 8;
        const uint64_t sp32 = (1ull << w32) - 1, sp8 = (1ull << w8) - 1;
        const std::vector<uint64_t> rc = residuals(r, w32, n, INT32_MIN + int64_t(r() % ((1ull << 32) - sp32)));
        const std::vector<uint64_t> len = residuals(r, w32, n, int64_t(r() % ((1ull << 32) - sp32)));
        const std::vector<uint64_t> sub = residuals(r, w8, n, int64_t(r() % (256 - sp8)));
        // VAR_OFF is u32 DELTA: steps in [-2^(w32-1), 2^(w32-1) - 1], both ends present, each drawn
        // from the part of that range that keeps the offset a u32 (it always holds 0)
        const int64_t olo = w32 ? -(int64_t(1) << (w32 - 1)) : 0, ohi = w32 ? (int64_t(1) << (w32 - 1)) - 1 : 0;
        Rows rows;
        uint64_t x1 = r(), x0 = r();
        int64_t off = int64_t(1) << 31;
        for (size_t i = 0; i < n; ++i) {
          if (i) x1 += d1[i - 1];
          if (kind && i) x0 += d0[i - 1];
          if (i == 1) off += olo;
          else if (i == 2) off += ohi;
          else if (i) {
            const int64_t a = olo > -off ? olo : -off, b = ohi < int64_t(UINT32_MAX) - off ? ohi : int64_t(UINT32_MAX) - off;
            off += a + int64_t(r() % uint64_t(b - a + 1));
          }
          rows.add(kind, int32_t(int64_t(rc[i])), int64_t(x1), uint32_t(off), uint32_t(len[i]), uint8_t(sub[i]),
                   kind ? int64_t(x0) : int64_t(d0[i]), uint32_t(r() % 2));
        }
        Out* o = check(rows);
        const uint32_t s = 2 + 6 * kind;
        REQUIRE(width_of(o->p, s + 1) == w && width_of(o->p, s + 5) == w);
        REQUIRE(width_of(o->p, s + 0) == w32 && width_of(o->p, s + 3) == w32 && width_of(o->p, s + 4) == w8);
        REQUIRE(width_of(o->p, s + 2) == w32);
        delete o;
      }
}

void extremes() {
  Rows rows;
  const int64_t pat[] = {INT64_MIN, INT64_MAX, INT64_MIN, 0, INT64_MAX, INT64_MAX, INT64_MIN, -1, 1};
  for (int k = 0; k < 300; ++k)
    for (int64_t v : pat)
      rows.add(uint32_t(k % 4), (k / 4) % 2 ? INT32_MIN : INT32_MAX, v, k % 3 ? 0u : UINT32_MAX, k % 5 ? UINT32_MAX : 0u, uint8_t((k / 4) % 2 ? 255 : 0), v);
  Out* o = check(rows);
  REQUIRE(width_of(o->p, 2 + 5) == 64 && width_of(o->p, 2 + 6 + 5) == 64 && width_of(o->p, 2 + 0) == 32 && width_of(o->p, 2 + 3) == 32);
  delete o;
}

void bad_rows() {
  std::mt19937_64 r(0xBAD0);
  Rows rows = mixed(r, 2500);
  const clg_columns in = rows.c();
  const Ref want = reference(rows);
  Rows broken = rows;
  broken.idx[2400] = uint32_t(rows.tag.size());      // w_idx == n_rec
  broken.idx[37] = uint32_t(rows.tag.size()) + 5;
  broken.tag[broken.idx[36]] = 2;                    // a narrow tag
  broken.tag[broken.idx[1999]] = 7;
  const clg_columns bin = broken.c();
  Out o(want.desc.size() + 64, want.bits.size() + 4096);
  REQUIRE(clg::wpack_build_host(&bin, &o.p) == CLG_E_INVALID_ARG && o.p.bad_row == 36 && o.untouched());
  REQUIRE(o.p.n_bits == 0 && o.p.blk_base[26] == 0);
  broken.tag[broken.idx[36]] = rows.tag[rows.idx[36]];
  REQUIRE(clg::wpack_build_host(&bin, &o.p) == CLG_E_INVALID_ARG && o.p.bad_row == 37 && o.untouched());
  broken.idx[37] = rows.idx[37];
  REQUIRE(clg::wpack_build_host(&bin, &o.p) == CLG_E_INVALID_ARG && o.p.bad_row == 1999 && o.untouched());
  clg_packed_wide sizes{};
  REQUIRE(clg::wpack_build_host(&bin, &sizes) == CLG_E_INVALID_ARG && sizes.bad_row == 1999);
  REQUIRE(clg::wpack_build_host(&in, &o.p) == CLG_OK && o.p.bad_row == ~0ull);
  // the pack's own argument checks
  clg_packed_wide p{};
  REQUIRE(clg::wpack_build_host(nullptr, &p) == CLG_E_INVALID_ARG && clg::wpack_build_host(&in, nullptr) == CLG_E_INVALID_ARG);
  clg_columns nul = in;
  nul.w_sub = nullptr;
  REQUIRE(clg::wpack_build_host(&nul, &p) == CLG_E_INVALID_ARG);
  nul = in, nul.tag = nullptr;
  REQUIRE(clg::wpack_build_host(&nul, &p) == CLG_E_INVALID_ARG);
}

// Every rejection of clg_unpack_wide_host: its report, and the output untouched.
void malformed() {
  std::mt19937_64 r(0xBAD);
  const Rows rows = mixed(r, 2500);
  Out* o = check(rows);
  const clg_packed_wide good = o->p;
  const auto rejects = [&](const clg_packed_wide& p, uint32_t what, uint32_t stream, uint64_t block) {
    Back b(2500);
    clg_unpack_bad bad;
    REQUIRE(clg::wpack_unpack_host(&p, &b.c, &bad) == CLG_E_INVALID_ARG);
    REQUIRE(bad.what == what && bad.stream == stream && bad.block == block);
    REQUIRE(b.untouched());
    REQUIRE(clg::wpack_unpack_host(&p, &b.c, nullptr) == CLG_E_INVALID_ARG && b.untouched());
  };
  const auto poke = [&](uint64_t blk, auto&& f, uint32_t what, uint32_t stream, uint64_t block) {
    const clg_pack_block keep = o->desc[blk];
    f(o->desc[blk]);
    rejects(good, what, stream, block);
    o->desc[blk] = keep;
  };
  const uint32_t L = CLG_UNPACK_BAD_LAYOUT, B = CLG_UNPACK_BAD_BLOCK, V = CLG_UNPACK_BAD_VALUE;
  clg_packed_wide p;
  // layout: the narrow pack's rules over 26 streams
  p = good, p.blk_base[0] = 1; rejects(p, L, 0, 0);
  p = good, p.blk_base[8] += 1; rejects(p, L, 7, 0);
  p = good, p.blk_base[3] = p.blk_base[4] + 1; rejects(p, L, 2, 0);
  p = good, p.n_val[9] += 1024; rejects(p, L, 9, 0);
  p = good, p.cap_desc = p.blk_base[26] - 1; rejects(p, L, 0, 0);
  p = good, p.n_bits = p.cap_bits + 16; rejects(p, L, 0, 0);
  p = good, p.desc = nullptr; rejects(p, L, 0, 0);
  p = good, p.bits = nullptr; rejects(p, L, 0, 0);
  // layout: the wide rows' own rules (lengths moved inside their last block, so the block counts still agree)
  REQUIRE(good.n_val[0] == 2500 && good.n_val[2] % 1024 > 1 && good.n_val[8] % 1024 > 1);
  p = good, p.n_val[1] -= 1; rejects(p, L, 1, 0);                      // KIND and IDX differ
  p = good, p.n_val[0] -= 1, p.n_val[1] -= 1; rejects(p, L, 0, 0);     // the kinds no longer sum to the rows
  p = good, p.n_val[2 + 3] -= 1; rejects(p, L, 2 + 3, 0);              // kind 0's VAR_LEN shorter than its RC
  p = good, p.n_val[2 + 6 + 5] += 1; rejects(p, L, 2 + 6 + 5, 0);      // kind 1's V0 longer
  p = good;  // a whole kind one shorter: the sum
  for (uint32_t f = 0; f < 6; ++f) p.n_val[2 + 12 + f] -= 1;
  rejects(p, L, 0, 0);
  // block
  const uint64_t bk = good.blk_base[0], bi = good.blk_base[1], b1 = good.blk_base[2 + 1];
  poke(bi + 1, [](clg_pack_block& d) { d.width = 65; }, B, 1, 1);
  poke(bk, [](clg_pack_block& d) { d.count = 1023; }, B, 0, 0);
  poke(bk + 2, [](clg_pack_block& d) { d.count = 453; }, B, 0, 2);
  poke(b1, [](clg_pack_block& d) { d.count = 0; }, B, 3, 0);
  poke(bi + 2, [&](clg_pack_block& d) { d.pos = good.n_bits; }, B, 1, 2);
  poke(bi + 2, [](clg_pack_block& d) { d.pos = ~0ull - 15; }, B, 1, 2);
  poke(bi, [](clg_pack_block& d) { d.pos += 8; }, B, 1, 0);  // not a multiple of 16
  p = good, p.n_bits = 16; rejects(p, B, 0, 0);
  // a block finding comes before a value finding, whatever their streams
  {
    const clg_pack_block keep = o->desc[bk];
    o->desc[bk].ref = 2;  // KIND up to 5
    poke(good.blk_base[20], [](clg_pack_block& d) { d.width = 70; }, B, 20, 0);
    o->desc[bk] = keep;
  }
  // value: a KIND of 4 and above, a histogram that differs, the elements' bounds
  REQUIRE(o->desc[bk + 1].width == 2);
  poke(bk + 1, [](clg_pack_block& d) { d.ref = 1; }, V, 0, 1);   // kinds 1 .. 4
  poke(bk, [](clg_pack_block& d) { d.ref = -1; }, V, 0, 0);      // a kind of -1
  {
    // two rows' kinds swapped for one kind: every KIND is a kind, the histogram differs
    Out* c = check(rows);
    uint8_t* payload = c->bits.data() + c->desc[bk].pos;
    const uint8_t k0 = payload[0] & 3;
    payload[0] = uint8_t((payload[0] & ~3) | ((k0 + 1) & 3));
    rejects(c->p, V, 0, 0);
    delete c;
  }
  const uint32_t s_rc = 2 + 0, s_off = 2 + 6 + 2, s_len = 2 + 12 + 3, s_sub = 2 + 18 + 4;
  poke(good.blk_base[s_rc], [](clg_pack_block& d) { d.ref = int64_t(INT32_MAX) - 5; }, V, s_rc, 0);
  poke(good.blk_base[s_rc], [](clg_pack_block& d) { d.ref = int64_t(INT32_MIN) - 1; }, V, s_rc, 0);
  poke(good.blk_base[s_off], [](clg_pack_block& d) { d.first = int64_t(UINT32_MAX) - 3; }, V, s_off, 0);  // u32 past 2^32 - 1
  poke(good.blk_base[s_off], [](clg_pack_block& d) { d.first = -1; }, V, s_off, 0);                       // u32 below 0
  poke(good.blk_base[s_len], [](clg_pack_block& d) { d.ref = int64_t(UINT32_MAX); }, V, s_len, 0);
  poke(good.blk_base[s_len], [](clg_pack_block& d) { d.ref = -1; }, V, s_len, 0);
  poke(good.blk_base[s_sub], [](clg_pack_block& d) { d.ref = 255; }, V, s_sub, 0);
  poke(good.blk_base[1] + 1, [](clg_pack_block& d) { d.first = int64_t(1) << 32; }, V, 1, 1);  // IDX
  // u32 values at the type's edges pass
  {
    Rows e;
    e.add(1, 0, 0, 0, UINT32_MAX, 0, 0), e.add(1, 0, 0, UINT32_MAX, 0, 0, 0), e.add(1, 0, 0, 0, UINT32_MAX, 0, 0);
    delete check(e);
  }
  // still good
  Back b(2500);
  clg_unpack_bad bad;
  REQUIRE(clg::wpack_unpack_host(&good, &b.c, &bad) == CLG_OK && b.equals(rows));
  REQUIRE(clg::wpack_unpack_host(nullptr, &b.c, &bad) == CLG_E_INVALID_ARG && clg::wpack_unpack_host(&good, nullptr, &bad) == CLG_E_INVALID_ARG);
  // some but not all of the seven arrays: nothing can be written
  Back part(2500);
  part.c.w_sub = nullptr;
  REQUIRE(clg::wpack_unpack_host(&good, &part.c, &bad) == CLG_E_CAPACITY && part.untouched());
  delete o;
}

// The scheme table is part of the format: held against the reference's copy.
void table() {
  for (uint32_t s = 0; s < 26; ++s) REQUIRE(clg::wpack_is_delta(s) == (kDelta[s] != 0));
  const uint32_t elem[6] = {clg::kElemI32, clg::kElemI64, clg::kElemU32, clg::kElemU32, clg::kElemU8, clg::kElemI64};
  REQUIRE(clg::wpack_stream_elem(0) == clg::kElemU8 && clg::wpack_stream_elem(1) == clg::kElemU32);
  for (uint32_t t = 0; t < 4; ++t)
    for (uint32_t f = 0; f < 6; ++f) REQUIRE(clg::wpack_stream_elem(clg::wpack_stream(t, f)) == elem[f] && clg::wpack_stream(t, f) == 2 + 6 * t + f);
}

}  // namespace

int main() {
  table();
  lengths();
  widths();
  extremes();
  bad_rows();
  malformed();
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
