// pack_wide.h -- packed wide rows: the format's one definition, for the kernels (pack_wide.hip),
// the engine and the CPU version.
//
// A wide row (w_idx, w_rc, w_v1, w_var_off, w_var_len, w_sub, w_v0) belongs to one of four record
// kinds, kind = tag[w_idx] - 3, and one w_* array mixes what the four kinds keep in it: stream
// lengths beside millisecond clocks beside checkpoint ids.  So the rows are partitioned by kind
// first (stable: rank r of kind t is the r-th row of that kind) and every field of every kind is a
// stream of its own; two more streams, the kinds and the w_idx of all rows in row order, let a
// reader put the rows back.  26 streams (kWPackStreams), each cut into blocks of kPackBlock values
// that are packed exactly as pack.h packs a block: residuals, ref, width, payload, padding.
//
//   stream 0 KIND, 1 IDX, then 2 + 6 * kind + field with the fields in kWPackField's order
//
// The element (what a value is extended from) and the scheme of a stream are kWPackField's and
// part of the format.  A field a kind never uses is all zeros and costs a width-0 descriptor per
// block; nothing about the values is assumed, so any w_* content round-trips.
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/wpack_host.cpp).
#pragma once
#include "pack.h"

namespace clg {

constexpr uint32_t kWPackKinds = CLG_WPACK_KINDS;
constexpr uint32_t kWPackFields = CLG_WPACK_FIELDS;
constexpr uint32_t kWPackStreams = CLG_WPACK_STREAMS;
constexpr uint32_t kWPackFirstTag = 3;  // kind = tag - kWPackFirstTag
static_assert(kWPackStreams == 2 + kWPackKinds * kWPackFields, "KIND, IDX and a stream per (kind, field)");

// A stream's element: what its values are extended to 64 bits from.
enum : uint32_t { kWElemU8 = 0, kWElemU32 = 1, kWElemI32 = 2, kWElemI64 = 3 };
enum : uint32_t { kWFor = 0, kWDelta = 1 };

// The scheme table.  V0 of kind 0 is a stream length (FOR); of kinds 1 - 3 a clock or a checkpoint
// id (DELTA).
struct WPackField {
  uint8_t elem, scheme_kind0, scheme_rest;
};
constexpr WPackField kWPackField[kWPackFields] = {
    {kWElemI32, kWFor, kWFor},      // RC       w_rc
    {kWElemI64, kWDelta, kWDelta},  // V1       w_v1
    {kWElemU32, kWDelta, kWDelta},  // VAR_OFF  w_var_off
    {kWElemU32, kWFor, kWFor},      // VAR_LEN  w_var_len
    {kWElemU8, kWFor, kWFor},       // SUB      w_sub
    {kWElemI64, kWFor, kWDelta},    // V0       w_v0
};
constexpr uint32_t kWPackKindElem = kWElemU8, kWPackKindScheme = kWFor;
constexpr uint32_t kWPackIdxElem = kWElemU32, kWPackIdxScheme = kWDelta;

// The table folded into two words (two bits of element and one of scheme a stream), so that device
// code indexes a constant and not an array.
constexpr uint64_t wpack_fold_elem() {
  uint64_t w = uint64_t(kWPackKindElem) | uint64_t(kWPackIdxElem) << 2;
  for (uint32_t t = 0; t < kWPackKinds; ++t)
    for (uint32_t f = 0; f < kWPackFields; ++f) w |= uint64_t(kWPackField[f].elem) << (2 * (2 + t * kWPackFields + f));
  return w;
}
constexpr uint32_t wpack_fold_scheme() {
  uint32_t w = kWPackKindScheme | kWPackIdxScheme << 1;
  for (uint32_t t = 0; t < kWPackKinds; ++t)
    for (uint32_t f = 0; f < kWPackFields; ++f)
      w |= uint32_t(t ? kWPackField[f].scheme_rest : kWPackField[f].scheme_kind0) << (2 + t * kWPackFields + f);
  return w;
}
constexpr uint64_t kWPackElemBits = wpack_fold_elem();
constexpr uint32_t kWPackSchemeBits = wpack_fold_scheme();

CLG_PACK_HD uint32_t wpack_stream(uint32_t kind, uint32_t field) { return 2 + kind * kWPackFields + field; }
CLG_PACK_HD uint32_t wpack_elem(uint32_t stream) { return uint32_t(kWPackElemBits >> (2 * stream)) & 3u; }
CLG_PACK_HD bool wpack_is_delta(uint32_t stream) { return (kWPackSchemeBits >> stream & 1u) != 0; }
CLG_PACK_HD uint32_t wpack_elem_bytes(uint32_t elem) { return elem == kWElemU8 ? 1u : elem == kWElemI64 ? 8u : 4u; }
CLG_PACK_HD uint32_t wpack_resid(bool delta, uint32_t m) { return delta && m ? m - 1 : m; }

// Value i of an array of `elem`, extended to 64 bits.
CLG_PACK_HD int64_t wpack_load(uint32_t elem, const void* col, uint64_t i) {
  switch (elem) {
    case kWElemU8: return int64_t(static_cast<const uint8_t*>(col)[i]);
    case kWElemU32: return int64_t(static_cast<const uint32_t*>(col)[i]);
    case kWElemI32: return int64_t(static_cast<const int32_t*>(col)[i]);
    default: return static_cast<const int64_t*>(col)[i];
  }
}
// The element's bounds, for the unpack's value check.
CLG_PACK_HD bool wpack_value_ok(uint32_t elem, int64_t v) {
  switch (elem) {
    case kWElemU8: return v >= 0 && v <= 255;
    case kWElemU32: return v >= 0 && v <= int64_t(UINT32_MAX);
    case kWElemI32: return v >= INT32_MIN && v <= INT32_MAX;
    default: return true;
  }
}
CLG_PACK_HD void wpack_store(uint32_t elem, void* col, uint64_t i, int64_t v) {
  switch (elem) {
    case kWElemU8: static_cast<uint8_t*>(col)[i] = uint8_t(v); break;
    case kWElemU32: static_cast<uint32_t*>(col)[i] = uint32_t(v); break;
    case kWElemI32: static_cast<int32_t*>(col)[i] = int32_t(v); break;
    default: static_cast<int64_t*>(col)[i] = v; break;
  }
}

// The row's kind, or kWPackKinds for a row that has none (w_idx past the tags, a narrow tag).
CLG_PACK_HD uint32_t wpack_kind_of(const uint8_t* tag, uint64_t n_rec, uint32_t idx) {
  if (idx >= n_rec) return kWPackKinds;
  const uint32_t kind = uint32_t(tag[idx]) - kWPackFirstTag;
  return kind < kWPackKinds ? kind : kWPackKinds;
}

// The six field arrays of a clg_columns, in kWPackField's order.
struct WPackCols {
  void* col[kWPackFields];
};
inline WPackCols wpack_cols(const clg_columns& c) {
  return WPackCols{{c.w_rc, c.w_v1, c.w_var_off, c.w_var_len, c.w_sub, c.w_v0}};
}

inline void wpack_reset_result(clg_packed_wide* out) {
  for (uint32_t c = 0; c < kWPackStreams; ++c) out->n_val[c] = 0;
  for (uint32_t c = 0; c <= kWPackStreams; ++c) out->blk_base[c] = 0;
  out->n_bits = 0;
  out->bad_row = ~0ull;
}
inline bool wpack_sizes_only(const clg_packed_wide& p) { return !p.desc && !p.bits; }
// n_val and blk_base from the rows and the kinds' totals.
inline void wpack_layout(uint64_t n_wide, const uint64_t tot[kWPackKinds], clg_packed_wide* out) {
  out->n_val[CLG_WPACK_KIND] = out->n_val[CLG_WPACK_IDX] = n_wide;
  for (uint32_t t = 0; t < kWPackKinds; ++t)
    for (uint32_t f = 0; f < kWPackFields; ++f) out->n_val[wpack_stream(t, f)] = tot[t];
  out->blk_base[0] = 0;
  for (uint32_t c = 0; c < kWPackStreams; ++c) out->blk_base[c + 1] = out->blk_base[c] + pack_blocks(out->n_val[c]);
}
// The first output that is too small (its name), or null.
inline const char* wpack_short(const clg_packed_wide& p) {
  if ((p.desc ? p.cap_desc : 0) < p.blk_base[kWPackStreams]) return "desc";
  if ((p.bits ? p.cap_bits : 0) < p.n_bits) return "bits";
  return nullptr;
}

// One block's measure over m extended values: the descriptor but for pos.
inline clg_pack_block wpack_measure_block(const int64_t* x, uint32_t m, bool delta) {
  clg_pack_block b{};
  b.count = m;
  const uint32_t k = wpack_resid(delta, m);
  if (delta && m) b.first = x[0];
  if (!k) return b;
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (uint32_t i = delta ? 1 : 0; i < m; ++i) {
    const int64_t r = delta ? int64_t(uint64_t(x[i]) - uint64_t(x[i - 1])) : x[i];
    lo = r < lo ? r : lo;
    hi = r > hi ? r : hi;
  }
  b.ref = lo;
  b.width = pack_width(uint64_t(hi) - uint64_t(lo));
  return b;
}
// One block's payload into dst (pack_payload_bytes(k, width) bytes, written whole).
inline void wpack_write_block(const int64_t* x, const clg_pack_block& b, bool delta, uint8_t* dst) {
  const uint32_t k = wpack_resid(delta, b.count), w = b.width;
  const uint32_t bytes = pack_payload_bytes(k, w);
  if (!bytes) return;
  memset(dst, 0, bytes);
  uint64_t bit = 0;
  for (uint32_t i = delta ? 1 : 0; i < b.count; ++i, bit += w) {
    const uint64_t r = delta ? uint64_t(x[i]) - uint64_t(x[i - 1]) : uint64_t(x[i]);
    const uint64_t p = r - uint64_t(b.ref);
    const uint32_t sh = uint32_t(bit & 63);
    uint8_t* at = dst + (bit >> 6) * 8;
    uint64_t word;
    memcpy(&word, at, 8);
    word |= p << sh;
    memcpy(at, &word, 8);
    if (sh + w > 64) {  // (sh > 0 here: no shift by 64)
      memcpy(&word, at + 8, 8);
      word |= p >> (64 - sh);
      memcpy(at + 8, &word, 8);
    }
  }
}

// The packed wide rows of host columns (clg_pack_wide_host): the split by kind, a measure pass
// over each stream, then the write pass once the sizes are known to fit.
inline int wpack_build_host(const clg_columns* in, clg_packed_wide* out, const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  wpack_reset_result(out);
  const uint64_t nw = in->n_class[4], nr = in->n_rec;
  const WPackCols cols = wpack_cols(*in);
  if (nw) {
    if (!in->w_idx || !in->tag) return *what = "null input array", CLG_E_INVALID_ARG;
    for (uint32_t f = 0; f < kWPackFields; ++f)
      if (!cols.col[f]) return *what = "null input array", CLG_E_INVALID_ARG;
  }
  // the split: every stream's values, extended
  std::vector<int64_t> val[kWPackStreams];
  val[CLG_WPACK_KIND].reserve(size_t(nw)), val[CLG_WPACK_IDX].reserve(size_t(nw));
  uint64_t tot[kWPackKinds] = {};
  for (uint64_t k = 0; k < nw; ++k) {
    const uint32_t kind = wpack_kind_of(in->tag, nr, in->w_idx[k]);
    if (kind >= kWPackKinds) return out->bad_row = k, *what = "a row's w_idx or tag is not a wide record's", CLG_E_INVALID_ARG;
    val[CLG_WPACK_KIND].push_back(int64_t(kind));
    val[CLG_WPACK_IDX].push_back(int64_t(in->w_idx[k]));
    for (uint32_t f = 0; f < kWPackFields; ++f)
      val[wpack_stream(kind, f)].push_back(wpack_load(kWPackField[f].elem, cols.col[f], k));
    ++tot[kind];
  }
  wpack_layout(nw, tot, out);
  const bool sizes_only = wpack_sizes_only(*out);
  std::vector<clg_pack_block> desc;
  if (!sizes_only) desc.reserve(size_t(out->blk_base[kWPackStreams]));
  uint64_t pos = 0;
  for (uint32_t c = 0; c < kWPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks(out->n_val[c]); ++b) {
      const uint64_t i0 = b * kPackBlock;
      const uint32_t m = uint32_t(out->n_val[c] - i0 < kPackBlock ? out->n_val[c] - i0 : kPackBlock);
      clg_pack_block d = wpack_measure_block(val[c].data() + i0, m, wpack_is_delta(c));
      d.pos = pos;
      pos += pack_payload_bytes(wpack_resid(wpack_is_delta(c), m), d.width);
      if (!sizes_only) desc.push_back(d);
    }
  out->n_bits = pos;
  if (sizes_only) return CLG_OK;
  if (const char* name = wpack_short(*out)) return *what = name, CLG_E_CAPACITY;
  for (uint32_t c = 0; c < kWPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks(out->n_val[c]); ++b) {
      const clg_pack_block& d = desc[size_t(out->blk_base[c] + b)];
      out->desc[out->blk_base[c] + b] = d;
      wpack_write_block(val[c].data() + b * kPackBlock, d, wpack_is_delta(c), out->bits + d.pos);
    }
  return CLG_OK;
}

// ---- a clg_packed_wide read as input (clg_unpack_wide_host) ----------------------------------
// Nothing is trusted.  The checks and their order are pack_unpack_all_host's: the layout, then the
// sizes and the capacity, then every block, then every value; each kind of finding is reported
// with its lowest (stream, block).  The layout has three rules of its own, and the values two:
//   layout  n_val[KIND] == n_val[IDX] (stream 1 otherwise); the six streams of one kind have equal
//           n_val (the lowest stream that differs from its kind's RC); the kinds' n_val sum to
//           n_val[KIND] (stream 0)
//   value   a KIND above 3 (stream 0, its block); KIND's histogram equal to the kinds' n_val
//           (stream 0, block 0; tested once every KIND is a kind, before the other streams' values)

inline bool wpack_layout_in_ok(const clg_packed_wide& p, uint32_t* stream) {
  *stream = 0;
  if (p.blk_base[0] != 0) return false;
  for (uint32_t c = 0; c < kWPackStreams; ++c)
    if (p.blk_base[c + 1] < p.blk_base[c] || p.blk_base[c + 1] - p.blk_base[c] != pack_blocks_of(p.n_val[c]))
      return *stream = c, false;
  if (p.cap_desc < p.blk_base[kWPackStreams] || p.cap_bits < p.n_bits) return false;
  if ((p.blk_base[kWPackStreams] && !p.desc) || (p.n_bits && !p.bits)) return false;
  if (p.n_val[CLG_WPACK_KIND] != p.n_val[CLG_WPACK_IDX]) return *stream = CLG_WPACK_IDX, false;
  uint64_t sum = 0;
  for (uint32_t t = 0; t < kWPackKinds; ++t) {
    const uint64_t n = p.n_val[wpack_stream(t, 0)];
    for (uint32_t f = 1; f < kWPackFields; ++f)
      if (p.n_val[wpack_stream(t, f)] != n) return *stream = wpack_stream(t, f), false;
    if (n > p.n_val[CLG_WPACK_KIND] - sum) return false;  // (the sum passes the rows: no wrap)
    sum += n;
  }
  return sum == p.n_val[CLG_WPACK_KIND];
}

CLG_PACK_HD bool wpack_block_in_ok(const clg_pack_block& d, bool delta, uint64_t b, uint64_t n, uint64_t n_bits) {
  const uint64_t nb = pack_blocks_of(n);
  if (b >= nb) return false;
  const uint32_t want = b + 1 < nb ? kPackBlock : uint32_t(n - b * kPackBlock);
  if (d.width > 64 || d.count < 1 || d.count > kPackBlock || d.count != want) return false;
  if (d.pos % 16) return false;
  const uint64_t bytes = pack_payload_bytes(wpack_resid(delta, d.count), d.width);
  return d.pos <= n_bits && bytes <= n_bits - d.pos;
}

// A well-formed block's values, extended, into x[0 .. count).
inline void wpack_unpack_block(const clg_pack_block& d, bool delta, const uint8_t* bits, int64_t* x) {
  const uint8_t* payload = bits + d.pos;
  if (delta) {
    uint64_t v = uint64_t(d.first);
    for (uint32_t i = 0; i < d.count; ++i) {
      if (i) v += pack_get(payload, d.width, i - 1) + uint64_t(d.ref);
      x[i] = int64_t(v);
    }
  } else {
    for (uint32_t i = 0; i < d.count; ++i) x[i] = int64_t(pack_get(payload, d.width, i) + uint64_t(d.ref));
  }
}

inline int wpack_unpack_host(const clg_packed_wide* in, clg_columns* out, clg_unpack_bad* bad, const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  pack_bad_reset(bad);
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  uint32_t stream;
  if (!wpack_layout_in_ok(*in, &stream))
    return *what = "blk_base, n_val, the capacities and the pointers disagree", pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
  const uint64_t nw = in->n_val[CLG_WPACK_KIND];
  out->n_class[4] = nw;
  const WPackCols cols = wpack_cols(*out);
  bool any = out->w_idx != nullptr, all = out->w_idx != nullptr;
  for (uint32_t f = 0; f < kWPackFields; ++f) any = any || cols.col[f], all = all && cols.col[f];
  if (!any) return CLG_OK;  // sizes only
  if ((!all && nw) || out->cap_wide < nw) return *what = "the wide rows' arrays are too small", CLG_E_CAPACITY;
  // every block, then every value
  for (uint32_t c = 0; c < kWPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks_of(in->n_val[c]); ++b)
      if (!wpack_block_in_ok(in->desc[in->blk_base[c] + b], wpack_is_delta(c), b, in->n_val[c], in->n_bits))
        return *what = "malformed block descriptor", pack_bad_set(bad, CLG_UNPACK_BAD_BLOCK, c, b);
  std::vector<int64_t> val[kWPackStreams];
  for (uint32_t c = 0; c < kWPackStreams; ++c) {
    val[c].resize(size_t(in->n_val[c]));
    const uint32_t elem = wpack_elem(c);
    for (uint64_t b = 0; b < pack_blocks_of(in->n_val[c]); ++b) {
      const clg_pack_block& d = in->desc[in->blk_base[c] + b];
      int64_t* x = val[c].data() + b * kPackBlock;
      wpack_unpack_block(d, wpack_is_delta(c), in->bits, x);
      for (uint32_t i = 0; i < d.count; ++i)
        if (!wpack_value_ok(elem, x[i]) || (c == CLG_WPACK_KIND && x[i] >= int64_t(kWPackKinds)))
          return *what = "a value outside the stream's type", pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, c, b);
    }
    if (c == CLG_WPACK_KIND) {
      uint64_t hist[kWPackKinds] = {};
      for (uint64_t k = 0; k < nw; ++k) ++hist[val[c][size_t(k)]];
      for (uint32_t t = 0; t < kWPackKinds; ++t)
        if (hist[t] != in->n_val[wpack_stream(t, 0)])
          return *what = "the kinds' counts differ from the streams' lengths", pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, 0, 0);
    }
  }
  // the writes: row k takes the next rank of its kind
  uint64_t rank[kWPackKinds] = {};
  for (uint64_t k = 0; k < nw; ++k) {
    const uint32_t kind = uint32_t(val[CLG_WPACK_KIND][size_t(k)]);
    const uint64_t r = rank[kind]++;
    out->w_idx[k] = uint32_t(val[CLG_WPACK_IDX][size_t(k)]);
    for (uint32_t f = 0; f < kWPackFields; ++f) wpack_store(kWPackField[f].elem, cols.col[f], k, val[wpack_stream(kind, f)][size_t(r)]);
  }
  return CLG_OK;
}

}  // namespace clg
