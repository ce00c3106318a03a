// encode_columns.h -- typed columns back to log bytes: what the encode kernels
// (encode_columns.hip), the engine and the CPU version share, written once.
//
// The inverse of the columns decode (columns.h, payload.h).  Inputs (clg_columns_in): tag in
// record order, one value column per class, the wide rows (w_rc, w_v1, w_var_len, w_sub, w_v0;
// w_idx optional and only checked), the payload column (pos, var) and span_base.  Record i's
// bytes are SimpleDeterminantEncoder's (SimpleDeterminantEncoder.java:124-323, as encode.hip
// restates them for the SoA row):
//
//   ORDER          [0][i8]                                             2
//   TIMESTAMP      [1][i64]                                            9
//   RNG            [2][i32]                                            5
//   BUFFER_BUILT   [7][i32]                                            5
//   SERIALIZABLE   [3][payload]                                        1 + len
//   TIMER_TRIGGER  [4][rc i32][v0 i64][sub u8]  sub == 6: [len i32][payload]   14 | 18 + len
//   SOURCE_CHECKP. [5][rc i32][v0 i64][v1 i64][sub & 0x7F][sub >> 7]  sub & 0x80: [len i32][payload]
//                                                                      23 | 27 + len
//   IGNORE_CHECKP. [6][rc i32][v0 i64]                                 13
//
// The value comes from the record's class column at its rank in that class; a wide record's
// fields from wide row k, its rank among the wide tags; its payload is var[pos[k] : + w_var_len[k]],
// read only where the format carries one.  Span s holds the records from the sum of span_base row s
// up to the sum of row s + 1.
//
// Errors (CLG_E_INVALID_ARG, nothing written; the first kind in this order, its lowest index):
//   TAG     a tag above 7                                                  the record
//   TOTALS  a class's tag count differs from n_class[c]                    the class
//   SPAN    span_base rows decrease, the last row is not n_class, or the class counts of the
//           tags before a span's first record are not its row             the span
//   ROW     pos[k] + w_var_len[k] > n_var (64 bits) for a row whose format carries a payload, or
//           w_idx given and w_idx[k] is not the k-th wide record           the row
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/encode_columns_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/clonos_engine.h"
#include "columns.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLG_ECOL_HD __host__ __device__ __forceinline__
#else
#define CLG_ECOL_HD inline
#endif

namespace clg {

// The write tile: kEcolTile records (the columns' own tile, so the count and scan passes are the
// columns'), given to a workgroup of kEcolTileThreads threads, kEcolPer records each,
// kEcolTileThreads apart -- more and shorter threads than the columns' 256 x 16, since a thread's
// records are a serial chain and the write pass's LDS allows two workgroups a CU whatever their
// size.  The tile is staged in an LDS buffer of kEcolLds bytes; a tile whose bytes
// (with the destination's misalignment, under 16) do not fit stores directly.  Two workgroups fit a
// CU's 160 KiB: 2 x (kEcolLds + a flag byte per 16 + about 3 KiB of scan words).
constexpr uint32_t kEcolTile = kColTile;
constexpr uint32_t kEcolTileThreads = 512;
constexpr uint32_t kEcolPer = kEcolTile / kEcolTileThreads;
constexpr uint32_t kEcolLds = 64 * 1024;
// Payloads of at least this many bytes go from var to the output by one wave (payload.h kPayWaveRow).
constexpr uint32_t kEcolWaveRow = 64;
constexpr uint64_t kEcolNone = ~0ull;
// The longest record without its payload (a SourceCheckpoint with a reference).
constexpr uint32_t kEcolMaxHead = 27;

static_assert(2 * (kEcolLds + kEcolLds / 16 + 4096) <= 160 * 1024, "two write workgroups fit a CU's LDS");
static_assert(kEcolTile * 9 + 16 <= kEcolLds, "a tile of fixed-length records is staged");

CLG_ECOL_HD bool ecol_wide(uint32_t tag) { return tag - 3u < 4u; }

// The format carries a payload for this wide row.
CLG_ECOL_HD bool ecol_has_payload(uint32_t tag, uint32_t sub) {
  return tag == CLG_TAG_SERIALIZABLE || (tag == CLG_TAG_TIMER_TRIGGER && sub == 6) ||
         (tag == CLG_TAG_SOURCE_CHECKPOINT && (sub & 0x80u));
}

// A record's bytes before its payload (0: a tag above 7).
CLG_ECOL_HD uint32_t ecol_head_len(uint32_t tag, uint32_t sub) {
  switch (tag) {
    case CLG_TAG_ORDER: return 2;
    case CLG_TAG_TIMESTAMP: return 9;
    case CLG_TAG_RNG:
    case CLG_TAG_BUFFER_BUILT: return 5;
    case CLG_TAG_SERIALIZABLE: return 1;
    case CLG_TAG_TIMER_TRIGGER: return sub == 6 ? 18 : 14;
    case CLG_TAG_SOURCE_CHECKPOINT: return (sub & 0x80u) ? 27 : 23;
    case CLG_TAG_IGNORE_CHECKPOINT: return 13;
    default: return 0;
  }
}

// A record's encoded length (var_len counts only where the format carries a payload).
CLG_ECOL_HD uint64_t ecol_len(uint32_t tag, uint32_t sub, uint32_t var_len) {
  return uint64_t(ecol_head_len(tag, sub)) + (ecol_has_payload(tag, sub) ? var_len : 0u);
}

// A row's payload lies inside var (64 bits: pos + len does not wrap for any pos a caller gives).
CLG_ECOL_HD bool ecol_row_ok(uint64_t pos, uint32_t var_len, uint64_t n_var) {
  return pos <= n_var && uint64_t(var_len) <= n_var - pos;
}

template <class P>
CLG_ECOL_HD void ecol_put_be(P p, uint64_t at, uint64_t v, uint32_t width) {
  for (uint32_t k = 0; k < width; ++k) p[at + k] = uint8_t(v >> (8u * (width - 1u - k)));
}

// A record's bytes before its payload into a byte sink (host memory, LDS or global memory):
// ecol_head_len(tag, sub) bytes at p[at].  v0: the record's value; rc / v1 / sub / var_len: its
// wide row (wide records only).
template <class P>
CLG_ECOL_HD void ecol_put_head(P p, uint64_t at, uint32_t tag, int64_t v0, int32_t rc, int64_t v1, uint32_t sub,
                               uint32_t var_len) {
  p[at] = uint8_t(tag);
  switch (tag) {
    case CLG_TAG_ORDER: p[at + 1] = uint8_t(v0); break;                      // :124-127
    case CLG_TAG_TIMESTAMP: ecol_put_be(p, at + 1, uint64_t(v0), 8); break;  // :145-148
    case CLG_TAG_RNG:                                                        // :167-170
    case CLG_TAG_BUFFER_BUILT: ecol_put_be(p, at + 1, uint64_t(v0), 4); break;  // :189-192
    case CLG_TAG_IGNORE_CHECKPOINT:                                          // :289-293
      ecol_put_be(p, at + 1, uint32_t(rc), 4);
      ecol_put_be(p, at + 5, uint64_t(v0), 8);
      break;
    case CLG_TAG_TIMER_TRIGGER:                                              // :202-213
      ecol_put_be(p, at + 1, uint32_t(rc), 4);
      ecol_put_be(p, at + 5, uint64_t(v0), 8);
      p[at + 13] = uint8_t(sub);
      if (sub == 6) ecol_put_be(p, at + 14, var_len, 4);
      break;
    case CLG_TAG_SOURCE_CHECKPOINT:                                          // :244-257
      ecol_put_be(p, at + 1, uint32_t(rc), 4);
      ecol_put_be(p, at + 5, uint64_t(v0), 8);
      ecol_put_be(p, at + 13, uint64_t(v1), 8);
      p[at + 21] = uint8_t(sub & 0x7Fu);
      p[at + 22] = uint8_t(sub >> 7);
      if (sub & 0x80u) ecol_put_be(p, at + 23, var_len, 4);
      break;
    default: break;  // SERIALIZABLE :316-323: the tag, then the stream
  }
}

inline uint32_t ecol_spans(const clg_columns_in& in) { return in.n_spans ? in.n_spans : 1u; }

inline uint64_t ecol_row_sum(const uint64_t* row) {
  uint64_t s = 0;
  for (uint32_t c = 0; c < kColClasses; ++c) s += row[c];
  return s;
}

// span_base as given: rows do not decrease and the last is n_class.  kEcolNone: fine (or no
// span_base: one span); else the lowest span whose row is wrong (the row above a decrease; n_spans
// for the last row).
inline uint64_t ecol_span_rows_bad(const clg_columns_in& in) {
  if (!in.n_spans || !in.span_base) return kEcolNone;
  for (uint32_t s = 0; s < in.n_spans; ++s)
    for (uint32_t c = 0; c < kColClasses; ++c)
      if (in.span_base[uint64_t(s) * kColClasses + c] > in.span_base[uint64_t(s + 1) * kColClasses + c]) return s;
  for (uint32_t c = 0; c < kColClasses; ++c)
    if (in.span_base[uint64_t(in.n_spans) * kColClasses + c] != in.n_class[c]) return in.n_spans;
  return kEcolNone;
}

inline void ecol_reset_result(clg_encoded* out) {
  out->n_bytes = 0;
  out->bad_what = CLG_ENC_BAD_NONE;
  out->bad_index = kEcolNone;
}

inline int ecol_bad(clg_encoded* out, uint32_t what, uint64_t index, const char** text, const char* msg) {
  out->n_bytes = 0;
  out->bad_what = what;
  out->bad_index = index;
  *text = msg;
  return CLG_E_INVALID_ARG;
}

// ---- clg_columns_in's arrays, in EcolIn's order (host only; columns.h kColArray's counterpart) ----
// len: the count the array's length follows -- class c's total (0 .. 4), or one of the three below.
// needed: null is an error when that count is not 0 (w_idx is optional; pos may be null when no row
// carries a payload: that is a ROW matter only when one does, and then pos is read).
enum : uint8_t { kEcolLenRec = 5, kEcolLenPos = 6, kEcolLenVar = 7 };  // n_rec; n_class[4] + 1; n_var
struct EcolArray {
  uint8_t width;  // element bytes
  uint8_t len;
  bool needed;
  size_t at;  // the member's offset in clg_columns_in
};
#define CLG_ECOL_ARRAY(m, width, len, needed) {width, len, needed, offsetof(clg_columns_in, m)}
constexpr int kEcolArrays = 13;
constexpr int kEcolNarrowArrays = 5;   // the leading ones, which a clg_packed gives: tag and the value columns
constexpr int kEcolPackedArrays = 12;  // ... and which the two packed forms give together: all but var
constexpr EcolArray kEcolArray[kEcolArrays] = {
    CLG_ECOL_ARRAY(tag, 1, kEcolLenRec, true), CLG_ECOL_ARRAY(order, 1, 0, true),     CLG_ECOL_ARRAY(timestamp, 8, 1, true),
    CLG_ECOL_ARRAY(rng, 4, 2, true),           CLG_ECOL_ARRAY(buffer_built, 4, 3, true), CLG_ECOL_ARRAY(w_rc, 4, 4, true),
    CLG_ECOL_ARRAY(w_v1, 8, 4, true),          CLG_ECOL_ARRAY(w_var_len, 4, 4, true), CLG_ECOL_ARRAY(w_sub, 1, 4, true),
    CLG_ECOL_ARRAY(w_v0, 8, 4, true),          CLG_ECOL_ARRAY(w_idx, 4, 4, false),    CLG_ECOL_ARRAY(pos, 8, kEcolLenPos, false),
    CLG_ECOL_ARRAY(var, 1, kEcolLenVar, true)};
#undef CLG_ECOL_ARRAY
inline uint64_t ecol_array_len(const clg_columns_in& in, int i) {
  const uint8_t len = kEcolArray[i].len;
  return len < kColClasses ? in.n_class[len] : len == kEcolLenRec ? in.n_rec : len == kEcolLenPos ? in.n_class[kColWide] + 1 : in.n_var;
}
inline uint64_t ecol_array_bytes(const clg_columns_in& in, int i) { return ecol_array_len(in, i) * kEcolArray[i].width; }
inline const void* ecol_in_ptr(const clg_columns_in& in, int i) {
  const void* p;
  memcpy(&p, reinterpret_cast<const char*>(&in) + kEcolArray[i].at, sizeof p);
  return p;
}
inline void ecol_in_set(clg_columns_in* in, int i, const void* p) {
  memcpy(reinterpret_cast<char*>(in) + kEcolArray[i].at, &p, sizeof p);
}

// Null arrays that the counts say are read.
inline bool ecol_args_ok(const clg_columns_in& in) {
  for (int i = 0; i < kEcolArrays; ++i)
    if (kEcolArray[i].needed && ecol_array_len(in, i) && !ecol_in_ptr(in, i)) return false;
  if (in.n_spans && !in.span_base) return false;
  if (in.in_kind != CLG_MEM_HOST && in.in_kind != CLG_MEM_DEVICE && in.in_kind != CLG_MEM_MAPPED) return false;
  return true;
}

// The encode on the CPU, every array host memory: a checking pass over the tags and rows (totals,
// lengths, span byte bases, the lowest bad index of each kind), then one writing pass.  The rules
// are clg_encode_columns'; *what (optional) receives a static text for the error.
inline int ecol_build_host(const clg_columns_in* inp, clg_encoded* out, const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!inp || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  ecol_reset_result(out);
  const clg_columns_in& in = *inp;
  if (!ecol_args_ok(in)) return *what = "null input array or unknown in_kind", CLG_E_INVALID_ARG;
  const uint64_t n = in.n_rec;
  const uint32_t ns = ecol_spans(in);

  // pass 0: the tags (totals, the lowest bad tag)
  uint64_t tot[kColClasses] = {0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t c = col_class(in.tag[i]);
    if (c == kColBad) return ecol_bad(out, CLG_ENC_BAD_TAG, i, what, "a tag above 7");
    ++tot[c];
  }
  for (uint32_t c = 0; c < kColClasses; ++c)
    if (tot[c] != in.n_class[c]) return ecol_bad(out, CLG_ENC_BAD_TOTALS, c, what, "a class's tag count differs from n_class");
  uint64_t bad_span = ecol_span_rows_bad(in);

  // pass 1: lengths, span byte bases, span rows against the tags, rows
  uint64_t at[kColClasses] = {0, 0, 0, 0, 0}, bytes = 0, bad_row = kEcolNone;
  uint32_t s = 0;
  const bool one = !in.n_spans;
  const auto boundary = [&](uint32_t r) {  // span r starts here (r == ns: the end)
    if (out->span_byte_base) out->span_byte_base[r] = bytes;
    if (one || bad_span != kEcolNone) return;
    for (uint32_t c = 0; c < kColClasses; ++c)
      if (in.span_base[uint64_t(r) * kColClasses + c] != at[c]) {
        bad_span = r;
        return;
      }
  };
  const auto starts_at = [&](uint32_t r, uint64_t i) {
    return one ? (r == 0 && i == 0) : ecol_row_sum(in.span_base + uint64_t(r) * kColClasses) == i;
  };
  if (bad_span == kEcolNone) {
    for (uint64_t i = 0; i < n; ++i) {
      while (s < ns && starts_at(s, i)) boundary(s++);
      const uint32_t t = in.tag[i], c = col_class(t);
      if (c >= kColClasses) continue;  // (pass 0 found none)
      const uint64_t k = at[c]++;
      if (c != kColWide) {
        bytes += ecol_head_len(t, 0);
        continue;
      }
      const uint32_t sub = in.w_sub[k], vl = in.w_var_len[k];
      if (bad_row == kEcolNone) {
        if (in.w_idx && in.w_idx[k] != i) bad_row = k;
        else if (ecol_has_payload(t, sub) && (!in.pos || !ecol_row_ok(in.pos[k], vl, in.n_var))) bad_row = k;
      }
      bytes += ecol_len(t, sub, vl);
    }
    // the spans that start at the end; a span whose row sum was passed over is bad (its row is
    // not the counts before any record)
    while (s < ns && starts_at(s, n)) boundary(s++);
    if (s < ns && bad_span == kEcolNone) bad_span = s;
    if (bad_span == kEcolNone) boundary(ns);
  }
  if (bad_span != kEcolNone) return ecol_bad(out, CLG_ENC_BAD_SPAN, bad_span, what, "span_base does not describe the tags");
  if (bad_row != kEcolNone) return ecol_bad(out, CLG_ENC_BAD_ROW, bad_row, what, "a wide row's payload passes n_var, or w_idx names another record");
  out->n_bytes = bytes;
  if (!out->bytes) return CLG_OK;  // sizes only
  if (out->cap < bytes) return *what = "bytes", CLG_E_CAPACITY;

  // pass 2: the write
  uint8_t* p = static_cast<uint8_t*>(out->bytes);
  uint64_t o = 0;
  for (uint32_t c = 0; c < kColClasses; ++c) at[c] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t t = in.tag[i], c = col_class(t);
    if (c >= kColClasses) continue;  // (pass 0 found none)
    const uint64_t k = at[c]++;
    switch (c) {
      case kColOrder: ecol_put_head(p, o, t, int64_t(in.order[k]), 0, 0, 0, 0); break;
      case kColTimestamp: ecol_put_head(p, o, t, in.timestamp[k], 0, 0, 0, 0); break;
      case kColRng: ecol_put_head(p, o, t, int64_t(in.rng[k]), 0, 0, 0, 0); break;
      case kColBufferBuilt: ecol_put_head(p, o, t, int64_t(in.buffer_built[k]), 0, 0, 0, 0); break;
      default: {
        const uint32_t sub = in.w_sub[k], vl = in.w_var_len[k];
        ecol_put_head(p, o, t, in.w_v0[k], in.w_rc[k], in.w_v1[k], sub, vl);
        if (ecol_has_payload(t, sub) && vl) memcpy(p + o + ecol_head_len(t, sub), in.var + in.pos[k], vl);
        o += ecol_len(t, sub, vl);
        continue;
      }
    }
    o += ecol_head_len(t, 0);
  }
  return CLG_OK;
}

}  // namespace clg
