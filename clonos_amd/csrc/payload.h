// payload.h -- the payload column of typed replay columns: what the payload kernels
// (payload.hip), the engine and the CPU version share, written once.
//
// A wide record's payload (a TimerTrigger's name, a SourceCheckpoint's storage reference, a
// Serializable record's Java stream) reaches a columns caller only as w_var_off / w_var_len,
// offsets into its span's bytes.  The payload column carries the bytes themselves, packed back
// to back in row order -- the shape clg_encode_in's `var` has on the encode side:
//
//   inputs   n_spans spans of bytes; wide rows 0 .. n_rows with w_var_off[k], w_var_len[k]
//            (span-relative, as the decode writes them); row_base[n_spans + 1], starting at 0,
//            not decreasing, its last entry n_rows: row k belongs to span s when
//            row_base[s] <= k < row_base[s + 1] (for columns: span_base[s * 5 + 4])
//   outputs  pos u64[n_rows + 1], the exclusive prefix sum of w_var_len (pos[n_rows] = n_var);
//            var u8[n_var], var[pos[k] : pos[k + 1]] = span_s[w_var_off[k] : + w_var_len[k]]
//
// A row of length 0 occupies nothing.  A row whose range passes its span's end is a bad row:
// CLG_E_INVALID_ARG, the lowest such row in bad_row, nothing written; it counts as length 0 in
// the size pass and none of its bytes is ever loaded.  var and pos both null: sizes only.  A
// capacity below its total: CLG_E_CAPACITY, the results filled, nothing written.
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/payload_host.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/clonos_engine.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLG_PAY_HD __host__ __device__ __forceinline__
#else
#define CLG_PAY_HD inline
#endif

namespace clg {

// Rows per tile: one workgroup of kPayThreads threads, kPayPerThread consecutive rows each (a
// thread's offsets and lengths are one 16-byte load each).
constexpr uint32_t kPayThreads = 256;
constexpr uint32_t kPayPerThread = 4;
constexpr uint32_t kPayTile = kPayThreads * kPayPerThread;  // 1024
// The scan pass is one workgroup of this many threads, a tile per thread and round.
constexpr uint32_t kPayScanThreads = 1024;
// Rows of at least this many bytes are copied by a wave, shorter ones by one lane.
constexpr uint32_t kPayWaveRow = 64;
constexpr uint64_t kPayNoRow = ~0ull;
// The one-launch form (k_pay_small: one workgroup of kPayScanThreads threads, four tiles a
// round) takes calls of at most this many rows whose spans hold at most this many bytes (an upper
// bound of n_var that the host knows); larger ones take the multi-kernel form.  kPaySmallRows is
// its floor, two rounds plus one row: the measured crossover is 2048 to 4096 rows of 41 bytes on average,
// and between the two the one-launch form loses.  kPaySmallBytes lies between the
// last payload size measured faster (81 KB) and the first measured slower (168 KB).
constexpr uint32_t kPaySmallRows = 8193;
constexpr uint32_t kPaySmallBytes = 131072;
static_assert(kPaySmallRows >= 2 * (kPayScanThreads / kPayThreads) * kPayTile + 1,
              "a test can reach the carry between the small kernel's rounds");

// A row's range lies inside its span (64-bit: off + len of two u32 does not wrap).
CLG_PAY_HD bool pay_row_ok(uint32_t off, uint32_t len, uint64_t span_len) { return uint64_t(off) + len <= span_len; }

// The span that holds row k < row_base[n_spans]: the last span that starts at or before it.
// Spans without rows have equal entries, so that span's next entry is above k.
CLG_PAY_HD uint32_t pay_span_of(const uint64_t* row_base, uint32_t lo, uint32_t hi, uint64_t k) {
  while (hi - lo > 1) {  // row_base[lo] <= k < row_base[hi]
    const uint32_t mid = lo + (hi - lo) / 2;
    if (row_base[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

// row_base starts at 0 and does not decrease (its last entry is the row count).
inline bool pay_row_base_ok(const uint64_t* row_base, uint32_t n_spans) {
  if (!n_spans) return true;
  if (!row_base || row_base[0] != 0) return false;
  for (uint32_t s = 0; s < n_spans; ++s)
    if (row_base[s] > row_base[s + 1]) return false;
  return true;
}

inline void pay_reset_result(clg_payloads* out) {
  out->n_rows = 0;
  out->n_var = 0;
  out->bad_row = kPayNoRow;
}

inline bool pay_sizes_only(const clg_payloads& p) { return !p.var && !p.pos; }

// The array whose capacity is below its total (its name), or null.  A null pointer holds nothing.
inline const char* pay_short(const clg_payloads& p, uint64_t n_rows, uint64_t n_var) {
  if ((p.pos ? p.cap_pos : 0) < n_rows + 1) return "pos";
  if ((p.var ? p.cap_var : 0) < n_var) return "var";
  return nullptr;
}

// The payload column of spans of one host buffer, on the CPU: span s is
// bytes[span_off[s], span_off[s] + span_len[s]).  The rules are the ones above; *what (optional)
// receives a static text for the error.
inline int pay_build_host(const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len, uint32_t n_spans,
                          const uint32_t* w_var_off, const uint32_t* w_var_len, const uint64_t* row_base,
                          clg_payloads* out, const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!out) return *what = "null argument", CLG_E_INVALID_ARG;
  pay_reset_result(out);
  if (n_spans && (!span_off || !span_len || !row_base)) return *what = "null argument", CLG_E_INVALID_ARG;
  if (!pay_row_base_ok(row_base, n_spans)) return *what = "row_base does not start at 0 or decreases", CLG_E_INVALID_ARG;
  const uint64_t n = n_spans ? row_base[n_spans] : 0;
  if (n && (!w_var_off || !w_var_len)) return *what = "null row array", CLG_E_INVALID_ARG;
  out->n_rows = n;

  // the size pass: the total, and the lowest bad row (it counts as length 0)
  uint64_t n_var = 0;
  uint32_t s = 0;
  for (uint64_t k = 0; k < n; ++k) {
    while (row_base[s + 1] <= k) ++s;
    if (!pay_row_ok(w_var_off[k], w_var_len[k], span_len[s])) {
      if (out->bad_row == kPayNoRow) out->bad_row = k;
    } else {
      n_var += w_var_len[k];
    }
  }
  out->n_var = n_var;
  if (out->bad_row != kPayNoRow) return *what = "a row's range passes its span's end", CLG_E_INVALID_ARG;
  if (pay_sizes_only(*out)) return CLG_OK;
  if (const char* name = pay_short(*out, n, n_var)) return *what = name, CLG_E_CAPACITY;
  if (n_var && !bytes) return *what = "null bytes", CLG_E_INVALID_ARG;

  // the write: every row is inside its span
  uint64_t at = 0;
  s = 0;
  for (uint64_t k = 0; k < n; ++k) {
    while (row_base[s + 1] <= k) ++s;
    out->pos[k] = at;
    if (w_var_len[k]) memcpy(out->var + at, bytes + span_off[s] + w_var_off[k], w_var_len[k]);
    at += w_var_len[k];
  }
  out->pos[n] = at;
  return CLG_OK;
}

}  // namespace clg
