// columns.h -- typed replay columns: what the column kernels (columns.hip), the engine and the
// CPU version share, written once.
//
// The decode's output is one row per record (off u32 | tag u8 | v0 i64, and a side row per wide
// record).  The replay consumers ask for one typed value at a time (LogReplayerImpl.java:61-119:
// a byte channel, an int random number, a long timestamp; SubpartitionRecoveryThread: int buffer
// sizes) and never for a record's byte offset.  The columns are the stable partition of a decoded
// batch by determinant class:
//
//   class          tags         column
//   ORDER        0 tag 0        order        i8[n_0]
//   TIMESTAMP    1 tag 1        timestamp    i64[n_1]
//   RNG          2 tag 2        rng          i32[n_2]
//   BUFFER_BUILT 3 tag 7        buffer_built i32[n_3]
//   WIDE         4 tags 3..6    the side table's rows, plus w_v0[k] = v0[w_idx[k]]
//
// Each column holds v0 of its class's records in record order, narrowed to the field's own width
// (lossless: the decode sign-extends those fields into v0).  tag u8[n] stays as it is, in record
// order: it is the interleaving.  span_base[(n_spans + 1) x 5] counts, per class, the records
// before each span; its last row holds the totals.
//
// `off` is NOT part of the columns: a caller that needs byte offsets keeps using the decode.
// Nothing else is lost: walking tag and popping each class's next value gives back tag, v0 and
// the side table exactly (col_to_soa below).
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/columns_host.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/clonos_engine.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLG_COL_HD __host__ __device__ __forceinline__
#else
#define CLG_COL_HD inline
#endif

namespace clg {

enum : uint32_t { kColOrder = 0, kColTimestamp = 1, kColRng = 2, kColBufferBuilt = 3, kColWide = 4, kColClasses = 5 };
constexpr uint32_t kColBad = 5;  // col_class of a tag above 7 (no column)

// Records per tile: one workgroup of kColThreads threads, kColPerThread records each.
constexpr uint32_t kColTile = 4096;
constexpr uint32_t kColThreads = 256;
constexpr uint32_t kColPerThread = kColTile / kColThreads;
// The scan pass is one workgroup of this many threads, a tile per thread and round.
constexpr uint32_t kColScanThreads = 1024;
// A tile's counts: a u32 per class, then the number of tags above 7, padded to 32 bytes.
constexpr uint32_t kColCountWords = 8;

// The one-launch form (k_col_small: one workgroup of kColScanThreads threads, four tiles a
// round) takes batches of at most this many records and spans; larger ones take the
// multi-kernel form.  kColSmallRecords is its floor, 8 tiles plus one (two rounds and a record, so
// that a test reaches the carry between rounds): the measured crossover is 16384 records, and
// between the two the one-launch form loses up to about 0.01 ms a call.
constexpr uint32_t kColSmallRecords = 32769;
constexpr uint32_t kColSmallSpans = 256;

static_assert(kColPerThread == 16, "a thread's tags are one 16-byte load");
static_assert(kColSmallRecords >= 8 * kColTile + 1, "a test can reach the carry between the small kernel's rounds");

CLG_COL_HD uint32_t col_class(uint32_t tag) {
  return tag <= CLG_TAG_RNG ? tag : tag == CLG_TAG_BUFFER_BUILT ? kColBufferBuilt : tag < CLG_TAG_BUFFER_BUILT ? kColWide : kColBad;
}

// The narrowing: v0 holds the field sign-extended, so the low bytes are the field.
CLG_COL_HD int8_t col_i8(int64_t v0) { return int8_t(uint8_t(uint64_t(v0))); }
CLG_COL_HD int32_t col_i32(int64_t v0) { return int32_t(uint32_t(uint64_t(v0))); }

// A column pointer's usable capacity: a null pointer holds nothing.
inline uint64_t col_cap(const void* p, uint64_t cap) { return p ? cap : 0; }

// The twelve arrays of a clg_columns in the struct's own order, which col_pack_offsets below and
// the small kernel's ColSmallOut share (col_ptr gives the pointer): the element width, the class whose total is its length
// (kColClasses: n_rec), and the name error texts give it.  The first five are the narrow columns;
// the seven wide arrays share one capacity and one name.
struct ColArray {
  uint32_t width, cls;
  const char* name;
};
constexpr int kColArrays = 12, kColNarrowArrays = 5;
constexpr ColArray kColArray[kColArrays] = {
    {1, kColClasses, "tag"}, {1, kColOrder, "order"}, {8, kColTimestamp, "timestamp"}, {4, kColRng, "rng"},
    {4, kColBufferBuilt, "buffer_built"}, {4, kColWide, "wide"}, {4, kColWide, "wide"}, {8, kColWide, "wide"},
    {4, kColWide, "wide"}, {4, kColWide, "wide"}, {1, kColWide, "wide"}, {8, kColWide, "wide"}};
inline void* col_ptr(const clg_columns& c, int i) {
  void* const p[kColArrays] = {c.tag,   c.order, c.timestamp, c.rng,       c.buffer_built, c.w_idx,
                               c.w_rc,  c.w_v1,  c.w_var_off, c.w_var_len, c.w_sub,        c.w_v0};
  return p[i];
}
// Array i's usable capacity, and its length in a batch of n records with the class totals tot.
inline uint64_t col_array_cap(const clg_columns& c, int i) {
  const uint64_t cap[6] = {c.cap_tag, c.cap_order, c.cap_timestamp, c.cap_rng, c.cap_buffer_built, c.cap_wide};
  return col_cap(col_ptr(c, i), cap[i < kColNarrowArrays ? i : kColNarrowArrays]);
}
inline uint64_t col_array_len(int i, uint64_t n, const uint64_t tot[kColClasses]) {
  return kColArray[i].cls == kColClasses ? n : tot[kColArray[i].cls];
}

inline bool col_sizes_only(const clg_columns& c) {
  for (int i = 0; i < kColArrays; ++i)
    if (col_ptr(c, i)) return false;
  return true;
}

// The first column whose capacity is below its total (its name), or null.
inline const char* col_short_column(const clg_columns& c, uint64_t n, const uint64_t tot[kColClasses]) {
  for (int i = 0; i < kColArrays; ++i)
    if (col_array_cap(c, i) < col_array_len(i, n, tot)) return kColArray[i].name;
  return nullptr;
}

// The packed layout of the twelve arrays (tag, order, timestamp, rng, buffer_built, w_idx, w_rc,
// w_v1, w_var_off, w_var_len, w_sub, w_v0) in one buffer: off[i] is array i's offset, a
// multiple of 16, and off[12] the end.
CLG_COL_HD void col_pack_offsets(uint64_t n, const uint64_t tot[kColClasses], uint64_t off[13]) {
  const uint64_t nw = tot[kColWide];
  const uint64_t bytes[12] = {n,      tot[kColOrder], 8 * tot[kColTimestamp], 4 * tot[kColRng], 4 * tot[kColBufferBuilt],
                              4 * nw, 4 * nw,         8 * nw,                 4 * nw,           4 * nw,
                              nw,     8 * nw};
  off[0] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 12; ++i) off[i + 1] = (off[i] + bytes[i] + 15) & ~uint64_t(15);
}
// An upper bound of col_pack_offsets' end that needs no totals.
inline uint64_t col_pack_bound(uint64_t n, uint64_t n_wide) { return 9 * n + 33 * n_wide + 13 * 16; }

inline void col_reset_result(clg_columns* out) {
  out->n_rec = 0;
  for (uint32_t c = 0; c < kColClasses; ++c) out->n_class[c] = 0;
  out->err_status = CLG_OK;
  out->err_span = 0;
  out->err_off = 0;
  out->err_tag = 0;
}

// span_rec_base must not decrease and must end inside the batch.
inline bool col_spans_ok(const uint64_t* span_rec_base, uint32_t n_spans, uint64_t n) {
  if (!n_spans) return true;
  if (!span_rec_base) return false;
  for (uint32_t s = 0; s < n_spans; ++s)
    if (span_rec_base[s] > span_rec_base[s + 1]) return false;
  return span_rec_base[n_spans] <= n;
}

// The span that holds record i (the last span that starts at or before it; 0 without spans).
inline uint32_t col_span_of(const uint64_t* span_rec_base, uint32_t n_spans, uint64_t i) {
  uint32_t lo = 0, hi = n_spans;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (span_rec_base[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// The columns of a decoded batch whose arrays are host memory, in one pass over the records.
// The rules are clg_columnize's:
//   * every column pointer null: sizes only (totals and span_base; no column written);
//   * a tag above 7: CLG_E_INVALID_ARG, the lowest such record index in err_off, nothing written;
//   * a column capacity below its total: CLG_E_CAPACITY, totals and span_base filled, no column
//     written (so nothing past any capacity);
//   * n_wide that is not the number of wide tags: CLG_E_INVALID_ARG.
// *what (optional) receives a static text for the error.
inline int col_build_host(const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans, clg_columns* out,
                          const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  col_reset_result(out);
  const uint64_t n = in->n_rec, nw = in->n_wide;
  if ((n && (!in->tag || !in->v0)) || (nw && !in->w_idx)) return *what = "null input array", CLG_E_INVALID_ARG;
  if (!col_spans_ok(span_rec_base, n_spans, n)) return *what = "span_rec_base decreases or passes n_rec", CLG_E_INVALID_ARG;

  // pass 0 (tags only): totals, span bases, the lowest bad tag
  uint64_t tot[kColClasses] = {0, 0, 0, 0, 0};
  uint32_t s = 0;
  const auto row = [&](uint32_t r) {
    if (out->span_base)
      for (uint32_t c = 0; c < kColClasses; ++c) out->span_base[uint64_t(r) * kColClasses + c] = tot[c];
  };
  for (uint64_t i = 0; i < n; ++i) {
    while (s < n_spans && span_rec_base[s] == i) row(s++);
    const uint32_t c = col_class(in->tag[i]);
    if (c == kColBad) {
      out->n_rec = n;
      out->err_status = CLG_E_INVALID_ARG;
      out->err_span = col_span_of(span_rec_base, n_spans, i);
      out->err_off = int64_t(i);
      out->err_tag = in->tag[i];
      return *what = "a tag above 7", CLG_E_INVALID_ARG;
    }
    ++tot[c];
  }
  while (s < n_spans) row(s++);  // (the spans that start at the end)
  row(n_spans);
  out->n_rec = n;
  for (uint32_t c = 0; c < kColClasses; ++c) out->n_class[c] = tot[c];
  if (tot[kColWide] != nw) return *what = "n_wide differs from the number of wide tags", CLG_E_INVALID_ARG;
  if (col_sizes_only(*out)) return CLG_OK;
  if (const char* name = col_short_column(*out, n, tot)) return *what = name, CLG_E_CAPACITY;

  // the one pass: every record's value to its class's next place
  uint64_t at[kColClasses] = {0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t t = in->tag[i];
    const int64_t v = in->v0[i];
    out->tag[i] = t;
    switch (col_class(t)) {
      case kColOrder: out->order[at[kColOrder]++] = col_i8(v); break;
      case kColTimestamp: out->timestamp[at[kColTimestamp]++] = v; break;
      case kColRng: out->rng[at[kColRng]++] = col_i32(v); break;
      case kColBufferBuilt: out->buffer_built[at[kColBufferBuilt]++] = col_i32(v); break;
      default: {
        const uint64_t k = at[kColWide]++;
        out->w_idx[k] = in->w_idx[k];
        out->w_rc[k] = in->w_rc[k];
        out->w_v1[k] = in->w_v1[k];
        out->w_var_off[k] = in->w_var_off[k];
        out->w_var_len[k] = in->w_var_len[k];
        out->w_sub[k] = in->w_sub[k];
        out->w_v0[k] = in->w_idx[k] < n ? in->v0[in->w_idx[k]] : 0;  // (= v when the row names its record)
      }
    }
  }
  return CLG_OK;
}

// The inverse: walk tag and pop each class's next value.  tag_out / v0_out hold n_rec entries
// (the side table is the columns' own w_* rows).  false: the tags ask for more values than a
// column holds.
inline bool col_to_soa(const clg_columns& c, uint8_t* tag_out, int64_t* v0_out) {
  uint64_t at[kColClasses] = {0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < c.n_rec; ++i) {
    const uint32_t k = col_class(c.tag[i]);
    if (k == kColBad || at[k] >= c.n_class[k]) return false;
    tag_out[i] = c.tag[i];
    const uint64_t j = at[k]++;
    v0_out[i] = k == kColOrder ? int64_t(c.order[j])
                : k == kColTimestamp ? c.timestamp[j]
                : k == kColRng ? int64_t(c.rng[j])
                : k == kColBufferBuilt ? int64_t(c.buffer_built[j])
                                       : c.w_v0[j];
  }
  for (uint32_t k = 0; k < kColClasses; ++k)
    if (at[k] != c.n_class[k]) return false;
  return true;
}

}  // namespace clg
