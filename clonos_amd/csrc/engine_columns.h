// engine_columns.h -- what the typed-columns family's three units share among themselves and with
// replay preparation (engine_replay.cpp).  Internal, like engine_impl.h: everything it declares has
// hidden visibility.  Who defines what:
//   engine_columns.cpp         decode -> columns: the placement helpers, columnize_device, decode_columns,
//                              decode_columns_var, gather_payloads_device, wide_row_base, pay_too_small, source_*
//   engine_pack.cpp            columns -> packed: pack_out_check, decode_columns_packed; the packed payload
//                              column both ways, nothing of which another unit calls
//   engine_encode_columns.cpp  columns -> log bytes, packed -> columns: nothing that another unit calls
//   here                       ColKeep, DecodeSource and carve
#pragma once
#include "engine_impl.h"
#include "pack.h"
#include "payload.h"
#include "placement.h"

#pragma GCC visibility push(hidden)

// ---- placement (placement.h): where the kernels of this family read and write ------------------
using clg::mem_kind_ok;
using clg::PlacePolicy;
using clg::PlaceSpec;

int place_arrays(const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what, clg::Placement* pl);
int copy_caller(clg_engine* e, void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind, uint32_t mem_kind = CLG_MEM_HOST);
int place_out(DevBuf& buf, const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what, clg::Placement* pl,
              size_t extra = 0);
int place_in(clg_engine* e, DevBuf& buf, const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what,
             clg::Placement* pl, size_t extra = 0);
int stage_out(clg_engine* e, const PlaceSpec* s, int n, const clg::Placement& pl);

// N pieces of engine scratch in `buf`, grown to them and 16 spare bytes (placement.h Carve).
template <int N>
int carve(DevBuf& buf, const uint64_t (&bytes)[N], clg::Carve<N>* c) {
  CHK(buf.ensure(clg::place_layout(bytes, N, c->off) + 16));
  c->base = buf.as<uint8_t>();
  return CLG_OK;
}

// ---- the decodes into typed columns ---------------------------------------------------------
// Replay preparation's columns form runs them once per batch: `run` decodes into the arrays it is
// given, `spans_of` gives the decoded spans to the payload gather.
using DecodeRun = std::function<int(clg_decoded*, uint64_t*)>;
using PaySpansOf = std::function<int(std::vector<clg::PaySpan>&, std::vector<uint32_t>&)>;
// keep (optional): the decoded batch in engine scratch and columnize_device's own status, for
// the payload column of the same rows (decode_columns_var) and the packed decodes.
struct ColKeep {
  clg_decoded d{};
  bool valid = false;        // the decode produced a batch and columnize_device ran
  int col_status = CLG_OK;   // columnize_device's
};
int decode_columns(clg_engine* e, const DecodeRun& run, uint32_t n_spans, clg_columns* out, ColKeep* keep = nullptr);
int decode_columns_var(clg_engine* e, const DecodeRun& run, uint32_t n, clg_columns* out, clg_payloads* var,
                       const PaySpansOf& spans_of);
int columnize_device(clg_engine* e, const clg_decoded& in, const uint64_t* span_rec_base, uint32_t n_spans, clg_columns* out);
int gather_payloads_device(clg_engine* e, const std::vector<clg::PaySpan>& spans, const std::vector<uint32_t>& segtab,
                           const uint32_t* d_off, const uint32_t* d_len, const uint64_t* row_base, clg_payloads* out,
                           bool sizes_forced = false, bool no_pos = false);
std::vector<uint64_t> wide_row_base(const uint64_t* span_base, uint32_t n);
int pay_too_small(const char* name, uint64_t rows, uint64_t bytes);

// What the decode-to-columns entry points decode, per source kind: `run` decodes it into the
// arrays it is given, `spans_of` gives its spans to the payload gather.
struct DecodeSource {
  DecodeRun run;
  PaySpansOf spans_of;
};
DecodeSource source_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n);
DecodeSource source_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len, uint32_t n);

// ---- packed outputs and inputs --------------------------------------------------------------
int pack_out_check(const clg::PackView& out, const char* what = "");  // (a packed input's, too)
// The packed decodes' one body, which replay preparation's packed form runs over its staged bytes:
// `run`'s batch as packed narrow columns in `out`, the wide rows plain in `wide` or (wpk) packed,
// and (var) their payloads from the spans `spans_of` gives.
int decode_columns_packed(clg_engine* e, const DecodeRun& run, uint32_t n, clg_columns* wide, clg_payloads* var,
                          clg_packed* out, const PaySpansOf& spans_of, clg_packed_wide* wpk = nullptr);

#pragma GCC visibility pop
