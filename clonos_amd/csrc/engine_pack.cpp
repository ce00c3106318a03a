// engine_pack.cpp -- the typed-columns family, columns -> packed: the five narrow columns bit-packed
// (pack.h), the wide rows packed by record kind (pack_wide.h) and the decodes that deliver either or
// both; clg_pack_columns*, clg_pack_wide* and clg_decode_{logs,host}_columns_packed[_wide].  The packed
// decodes run engine_columns.cpp's decode, columns and payload gather, once per batch each.  The
// packed payload column (ppay.h) is here both ways: clg_pack_payloads* and clg_unpack_payloads*.
#include "engine_columns.h"
#include "columns.h"
#include "pack.h"
#include "pack_wide.h"
#include "ppay.h"

// A packed output's memory kind and alignment (engine_columns.h: the unpacks check their input with it).
int pack_out_check(const clg::PackView& out, const char* what) {
  if (!mem_kind_ok(out.out_kind)) return fail(CLG_E_INVALID_ARG, "%sout_kind %u", what, out.out_kind);
  if (out.out_kind != CLG_MEM_HOST && (uintptr_t(out.desc) % 8 || uintptr_t(out.bits) % 16))
    return fail(CLG_E_INVALID_ARG, "desc must be aligned to 8 bytes and bits to 16");
  return CLG_OK;
}

namespace {

// ---- packed typed columns (pack.h) ----------------------------------------------------------
// The five narrow columns bit-packed where they lie: measure and the offset scan, the host's
// capacity check on the scan's total, then the write.  A LogReplayerImpl cursor
// (LogReplayerImpl.java:61-119) pops one typed value at a time from the blocks.

// What either form of the narrow pack starts with, over device-side streams: out's n_val and
// blk_base are filled, the streams checked and *pin filled from them.
int pack_prepare(const clg::PackSrc& src, clg_packed* out, clg::PackIn* pin) {
  clg::pack_reset_result(out);
  clg::pack_layout(src.n, out);
  const uint64_t nb = out->blk_base[clg::kPackStreams];
  if (nb >> 31) return fail(CLG_E_INVALID_ARG, "%llu blocks in one call", (unsigned long long)nb);
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) {
    if (src.n[c] && !src.col[c]) return fail(CLG_E_INVALID_ARG, "null input array (stream %u)", c);
    if (uintptr_t(src.col[c]) % clg::pack_stream_bytes(c))
      return fail(CLG_E_INVALID_ARG, "stream %u is not aligned to its element", c);
    pin->col[c] = src.col[c], pin->n[c] = src.n[c];
  }
  for (uint32_t c = 0; c <= clg::kPackStreams; ++c) pin->blk_base[c] = out->blk_base[c];
  return CLG_OK;
}
uint64_t pack_in_bytes(const clg::PackIn& pin) {
  uint64_t in_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) in_bytes += pin.n[c] * clg::pack_stream_bytes(c);
  return in_bytes;
}

// The multi-kernel form's measure and scan, after pack_prepare: out->n_bits is filled, the
// descriptors (with their offsets) are left in d_packdesc.
int pack_sizes(clg_engine* e, clg_packed* out, const clg::PackIn* pin) {
  const uint64_t nb = out->blk_base[clg::kPackStreams];
  const uint64_t in_bytes = pack_in_bytes(*pin);
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

// ---- what the two packed families share, over a PackView of either's struct ---------------------

// The write pass, after the sizes and the capacity check: device and registered outputs are
// written by the kernel, host ones through engine staging and one copy each.  launch(desc, bits):
// the family's write kernel over the placed outputs; in_bytes: what it reads of the values.
template <class Launch>
int pack_write(clg_engine* e, const clg::PackView& out, DevBuf& staging, const char* stat, uint64_t in_bytes,
               const Launch& launch) {
  const uint64_t nb = out.blocks(), nbits = *out.n_bits;
  if (!nb) return CLG_OK;
  const PlaceSpec dst[2] = {{out.desc, nb * sizeof(clg_pack_block), 8}, {out.bits, nbits, 16}};
  clg::Placement pl;
  CHK(place_out(staging, dst, 2, out.out_kind, PlacePolicy::stage_if_unresolved, "packed", &pl));
  CHK(e->timed(stat, in_bytes + nb * 64 + nbits, [&] { return launch(pl.at<clg_pack_block>(0), pl.at<uint8_t>(1)); }));
  CHK(stage_out(e, dst, 2, pl));
  return e->sync();
}

// prefix: "packed columns" or "packed wide rows".
int pack_capacity_error(const clg::PackView& out, const char* prefix, const char* name) {
  return fail(CLG_E_CAPACITY, "%s: %s is too small (blocks %llu, payload bytes %llu)", prefix, name,
              (unsigned long long)out.blocks(), (unsigned long long)*out.n_bits);
}

// Past the sizes: nothing more for the sizes-only call, the capacity error for a short output,
// else the write.
template <class Write>
int pack_finish(const clg::PackView& out, const char* prefix, const Write& write) {
  if (clg::pack_sizes_only(out)) return CLG_OK;
  if (const char* name = clg::pack_short(out)) return pack_capacity_error(out, prefix, name);
  return write();
}

int pack_write(clg_engine* e, const clg::PackIn& pin, const clg_packed* out) {
  uint64_t in_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) in_bytes += pin.n[c] * clg::pack_stream_bytes(c);
  const uint64_t nb = out->blk_base[clg::kPackStreams];
  const auto launch = [&](clg_pack_block* desc, uint8_t* bits) {
    return clg::launch_pack_write(pin, uint32_t(nb), e->d_packdesc.as<clg_pack_block>(), desc, bits, nb, out->n_bits, e->stream);
  };
  return pack_write(e, clg::pack_view(*out), e->d_packout, "pack_columns", in_bytes, launch);
}

// ---- packed wide rows (pack_wide.h) ---------------------------------------------------------
// Kind and count and the scan of the tile counts, the host's check of the bad-row word and its
// layout of the 26 streams from the four totals, the split into per-kind arrays in engine scratch,
// measure and the offset scan, the host's capacity check, then the write.

// Everything up to the sizes, over device-side rows: out's results are filled, the stream table is
// left in d_wpacktab and the descriptors (with their offsets) in d_wpackdesc.
int wpack_sizes(clg_engine* e, const clg::WPackSrc& src, clg_packed_wide* out) {
  clg::wpack_reset_result(out);
  const uint64_t nw = src.n_wide;
  if (nw >> 32) return fail(CLG_E_INVALID_ARG, "%llu wide rows in one call", (unsigned long long)nw);
  if (!nw) return CLG_OK;  // no rows: 26 empty streams, nothing to launch (a log without wide records pays nothing)
  const uint32_t nt = uint32_t((nw + clg::kWPackTile - 1) / clg::kWPackTile);
  const uint64_t kb[4] = {nw, uint64_t(nt) * clg::kWPackKinds * 4, uint64_t(nt) * clg::kWPackKinds * 8, 8};
  clg::Carve<4> ks;
  CHK(carve(e->d_wpackkind, kb, &ks));
  uint8_t* d_kind = ks.at<uint8_t>(0);
  uint32_t* d_cnt = ks.at<uint32_t>(1);
  uint64_t* d_base = ks.at<uint64_t>(2);
  unsigned long long* d_bad = ks.at<unsigned long long>(3);
  CHK(e->h_wpackres.ensure(sizeof(clg::WPackRes) + sizeof(clg::PackRes)));
  clg::WPackRes* res = e->h_wpackres.as<clg::WPackRes>();
  clg::PackRes* pres = reinterpret_cast<clg::PackRes*>(res + 1);
  // (bytes: w_idx, a tag and the kind byte a row; the tile counts written, read and their bases written)
  CHK(e->timed("pack_wide", nw * 6 + uint64_t(nt) * 64,
               [&] { return clg::launch_wpack_count_scan(src, nt, d_kind, d_cnt, d_base, d_bad, res, e->stream); }));
  CHK(e->sync());
  if (res->bad_row != ~0ull) {
    out->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "packed wide rows: row %llu's w_idx or tag is not a wide record's", (unsigned long long)res->bad_row);
  }
  if (res->tot[0] + res->tot[1] + res->tot[2] + res->tot[3] != nw) return fail(CLG_E_DEVICE, "packed wide rows: the kinds' totals do not sum to the rows");
  clg::wpack_layout(nw, res->tot, out);
  const uint64_t nb = out->blk_base[clg::kWPackStreams];

  // the per-kind arrays and the stream table
  constexpr int kArrays = int(clg::kWPackKinds * clg::kWPackFields);
  uint64_t cb[kArrays];
  clg::Carve<kArrays> so;
  for (uint32_t t = 0; t < clg::kWPackKinds; ++t)
    for (uint32_t f = 0; f < clg::kWPackFields; ++f)
      cb[t * clg::kWPackFields + f] = res->tot[t] * clg::pack_elem_bytes(clg::kWPackField[f].elem);
  CHK(carve(e->d_wpacksoa, cb, &so));
  CHK(e->h_wpacktab.ensure(sizeof(clg::WPackTab)));
  CHK(e->d_wpacktab.ensure(sizeof(clg::WPackTab)));
  clg::WPackTab* tab = e->h_wpacktab.as<clg::WPackTab>();
  tab->col[CLG_WPACK_KIND] = d_kind, tab->col[CLG_WPACK_IDX] = src.w_idx;
  for (int i = 0; i < kArrays; ++i) tab->col[2 + i] = so.at<uint8_t>(i);
  for (uint32_t c = 0; c < clg::kWPackStreams; ++c) tab->n[c] = out->n_val[c];
  for (uint32_t c = 0; c <= clg::kWPackStreams; ++c) tab->blk_base[c] = out->blk_base[c];
  HIPCHK(hipMemcpyAsync(e->d_wpacktab.p, tab, sizeof(clg::WPackTab), hipMemcpyHostToDevice, e->stream));
  const uint64_t ng = (nb + clg::kPackScanGroup - 1) / clg::kPackScanGroup;
  CHK(e->d_wpackdesc.ensure(size_t(nb) * sizeof(clg_pack_block) + 64));
  CHK(e->d_wpacksum.ensure(size_t(ng) * 8 + 64));
  // (bytes: the split reads a kind byte and 29 B a row and writes them; the measure reads the 26
  // streams, 34 B a row; a descriptor written, read and written again, the groups' sums)
  CHK(e->timed("pack_wide", nw * (1 + 29 + 29 + 34) + nb * 72 + ng * 24, [&] {
    const int st = clg::launch_wpack_split_measure(src, nt, d_kind, d_base, e->d_wpacktab.as<clg::WPackTab>(), uint32_t(nb),
                                                   e->d_wpackdesc.as<clg_pack_block>(), e->stream);
    if (st != CLG_OK) return st;
    return clg::launch_pack_scan(uint32_t(nb), e->d_wpackdesc.as<clg_pack_block>(), e->d_wpacksum.as<uint64_t>(), pres, e->stream);
  }));
  CHK(e->sync());
  out->n_bits = pres->n_bits;
  return CLG_OK;
}

int wpack_write(clg_engine* e, const clg_packed_wide* out) {
  const uint64_t nb = out->blk_base[clg::kWPackStreams];
  const auto launch = [&](clg_pack_block* desc, uint8_t* bits) {
    return clg::launch_wpack_write(e->d_wpacktab.as<clg::WPackTab>(), uint32_t(nb), e->d_wpackdesc.as<clg_pack_block>(), desc, bits,
                                   nb, out->n_bits, e->stream);
  };
  return pack_write(e, clg::pack_view(*out), e->d_wpackout, "pack_wide", out->n_val[CLG_WPACK_KIND] * 34, launch);
}

// ---- both packs in one launch of one workgroup (k_pack_small) ----------------------------------
// A narrow input of at most kPackSmallBlocks blocks and at most kWPackSmallRows wide rows, either
// or both: the kernel measures, scans, does the checks above itself and reports them in pinned
// memory, and writes.  One launch and one host sync (two for outputs the engine stages, whose
// size is known only then), where the multi-kernel forms take five and eight launches and two
// syncs each.  Every batch that the one-launch columns and payload forms take is taken here too.
static_assert(clg::kPackSmallBlocks >= (clg::kColSmallRecords + clg::kPackBlock - 1) / clg::kPackBlock +
                                           clg::kColSmallRecords / clg::kPackBlock + 4,
              "kPackSmallBlocks holds the five streams of kColSmallRecords records");
static_assert(clg::kWPackSmallRows >= clg::kPaySmallRows, "kWPackSmallRows holds the one-launch payload form's rows");

bool pack_small_takes(const clg_engine* e, const clg_packed& out) {
  return e->sw.pack_small && out.blk_base[clg::kPackStreams] <= clg::kPackSmallBlocks;
}
bool wpack_small_takes(const clg_engine* e, uint64_t n_wide) { return e->sw.pack_small && n_wide <= clg::kWPackSmallRows; }

// Where the kernel writes one half: the caller's device arrays, the device side of registered host
// arrays, or engine staging (desc | bits in one piece) of at most blocks_bound descriptors and
// bits_bound payload bytes.  The registry is asked for each array's capacity: the lengths are
// known only after the one launch.
int pack_small_place(const clg::PackView& v, DevBuf& staging, uint64_t blocks_bound, uint64_t bits_bound,
                     clg::PackSmallOut* o) {
  *o = clg::PackSmallOut{};
  if (clg::pack_sizes_only(v)) return CLG_OK;
  o->write = 1;
  const uint64_t cap_desc = v.desc ? v.cap_desc : 0, cap_bits = v.bits ? v.cap_bits : 0;
  // (CLG_MEM_MAPPED: a caller whose stated capacity passes the end of its registered range is staged
  // and copied, where the multi-kernel form, which knows the lengths by then, writes in place)
  const PlaceSpec dst[2] = {{v.desc, cap_desc * sizeof(clg_pack_block), 8}, {v.bits, cap_bits, 16}};
  clg::Placement pl;
  CHK(place_arrays(dst, 2, v.out_kind, PlacePolicy::stage_if_unresolved, "packed", &pl));
  if (!pl.staged()) {
    o->desc = pl.at<clg_pack_block>(0), o->bits = pl.at<uint8_t>(1);
    o->cap_desc = cap_desc, o->cap_bits = cap_bits;
    return CLG_OK;
  }
  o->cap_desc = std::min(cap_desc, blocks_bound), o->cap_bits = std::min(cap_bits, bits_bound);
  CHK(staging.ensure(o->cap_desc * sizeof(clg_pack_block) + o->cap_bits + 16));
  o->desc = staging.as<clg_pack_block>();
  o->packed = 1;
  return CLG_OK;
}

// pin, nout: the narrow half after pack_prepare (null: none).  wsrc, wout: the wide half, at least
// one row (null: none).  hold: nothing is written whatever the outputs say, and every size is still
// filled.  *short_cap (optional): the first capacity that is (hold: would be) short, as
// PackSmallRes has it.
struct PackSmallCall {
  const clg::PackIn* pin = nullptr;
  clg_packed* nout = nullptr;
  const clg::WPackSrc* wsrc = nullptr;
  clg_packed_wide* wout = nullptr;
  bool hold = false;
};
int pack_small(clg_engine* e, const PackSmallCall& c, uint32_t* short_cap = nullptr) {
  clg::PackSmallArgs a{};
  const uint64_t nw = c.wsrc ? c.wsrc->n_wide : 0;
  uint64_t moved = 0;
  if (c.pin) a.narrow = *c.pin, moved += 2 * pack_in_bytes(*c.pin);
  if (c.wsrc) {
    a.wide = *c.wsrc;
    CHK(e->d_wpackkind.ensure(nw + 16));
    CHK(e->d_wpacksoa.ensure(clg::wpack_soa_field(clg::kWPackFields, nw) + 16));
    a.d_kind = e->d_wpackkind.as<uint8_t>(), a.d_soa = e->d_wpacksoa.as<uint8_t>();
    moved += nw * (6 + 1 + 29 + 29 + 34 + 34);  // (kinds, the split in and out, the streams read twice)
  }
  a.sizes_only = c.hold ? 1u : 0u;
  clg::PackView nv{}, wv{};
  if (c.pin) {
    nv = clg::pack_view(*c.nout);
    CHK(pack_small_place(nv, e->d_packout, nv.blocks(), clg::pack_bits_bound_narrow(c.pin->n), &a.out_narrow));
  }
  if (c.wsrc) {
    wv = clg::pack_view(*c.wout);
    CHK(pack_small_place(wv, e->d_wpackout, clg::wpack_blocks_bound(nw), clg::wpack_bits_bound(nw), &a.out_wide));
  }
  CHK(e->h_packsmall.ensure(sizeof(clg::PackSmallRes)));
  clg::PackSmallRes* res = e->h_packsmall.as<clg::PackSmallRes>();
  e->stats["pack_small"].launches++;
  // The launch's time stands under the stat of the half that is most of it: the wide rows' where
  // there are any (kinds, split and 26 streams against five), else the narrow columns'.
  const bool timed_wide = c.wsrc != nullptr;
  CHK(e->timed(timed_wide ? "pack_wide" : "pack_columns", moved, [&] { return clg::launch_pack_small(a, res, e->stream); }));
  CHK(e->sync());
  if (e->cfg.flags & CLG_F_TIMING) {
    // `launches` of the two stats is a count of passes, not of kernels: the multi-kernel forms time
    // sizes and write of the narrow half and kinds, sizes and write of the wide one as a section
    // each.  The one launch did the same passes; the one above is timed, the others are counted here
    // with no time of their own, so that a reader of either stat sees the work that was done for
    // that half.  How many real launches there were is `pack_small`.
    const bool wrote = res->verdict == clg::kPackSmallWritten;
    if (c.pin) e->stats["pack_columns"].launches += (timed_wide ? 1 : 0) + (wrote && a.out_narrow.write ? 1 : 0);
    if (c.wsrc) e->stats["pack_wide"].launches += 1 + (wrote && a.out_wide.write ? 1 : 0);
  }
  if (short_cap) *short_cap = res->short_cap;
  if (res->verdict == clg::kPackSmallBadRow) {
    c.wout->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "packed wide rows: row %llu's w_idx or tag is not a wide record's", (unsigned long long)res->bad_row);
  }
  if (res->verdict > clg::kPackSmallCapacity) return fail(CLG_E_DEVICE, "the one-launch pack's verdict is %u", res->verdict);
  if (c.pin) c.nout->n_bits = res->n_bits[0];
  if (c.wsrc) {
    if (res->tot[0] + res->tot[1] + res->tot[2] + res->tot[3] != nw) return fail(CLG_E_DEVICE, "packed wide rows: the kinds' totals do not sum to the rows");
    clg::wpack_layout(nw, res->tot, c.wout);
    c.wout->n_bits = res->n_bits[1];
  }
  if (res->verdict == clg::kPackSmallCapacity) {
    const bool narrow = res->short_cap < 2;
    const clg::PackView& v = narrow ? nv : wv;
    const char* name = res->short_cap & 1 ? "bits" : "desc";
    if (!clg::pack_short(v)) return fail(CLG_E_DEVICE, "the one-launch pack's staging is too small (%s)", name);
    return pack_capacity_error(v, narrow ? "packed columns" : "packed wide rows", name);
  }
  if (res->verdict != clg::kPackSmallWritten) return CLG_OK;
  // staged halves come back in one copy each: desc | bits, exactly what was written
  const clg::PackSmallOut* so[2] = {&a.out_narrow, &a.out_wide};
  const clg::PackView* vs[2] = {&nv, &wv};
  uint64_t bytes[2] = {0, 0}, at[2] = {0, 0}, total = 0;
  for (int h = 0; h < 2; ++h)
    if (so[h]->write && so[h]->packed) {
      bytes[h] = vs[h]->blocks() * sizeof(clg_pack_block) + *vs[h]->n_bits;
      at[h] = total, total += (bytes[h] + 15) & ~uint64_t(15);
    }
  if (!total) return CLG_OK;
  CHK(e->h_packland.ensure(total));
  for (int h = 0; h < 2; ++h)
    if (bytes[h]) HIPCHK(hipMemcpyAsync(e->h_packland.as<uint8_t>() + at[h], so[h]->desc, bytes[h], hipMemcpyDeviceToHost, e->stream));
  CHK(e->sync());
  for (int h = 0; h < 2; ++h)
    if (bytes[h]) {
      const uint64_t db = vs[h]->blocks() * sizeof(clg_pack_block);
      const uint8_t* land = e->h_packland.as<uint8_t>() + at[h];
      if (db) memcpy(const_cast<clg_pack_block*>(vs[h]->desc), land, db);
      if (*vs[h]->n_bits) memcpy(const_cast<uint8_t*>(vs[h]->bits), land + db, *vs[h]->n_bits);
    }
  return CLG_OK;
}


// ---- the packed payload column (ppay.h) -----------------------------------------------------
// The pack: lcp and the scan, the host's checks on the scan's results (the lowest bad row, the
// capacities), then the write.  The unpack: the check and the scan, the host's reading of the
// findings and the totals, then the write; invalid input writes nothing.

// A packed payload column's memory kind and alignment, as an output or an input.
int ppay_kind_check(const clg_packed_payloads& p, const char* what) {
  if (!mem_kind_ok(p.out_kind)) return fail(CLG_E_INVALID_ARG, "%sout_kind %u", what, p.out_kind);
  if (p.out_kind != CLG_MEM_HOST && (uintptr_t(p.desc) % 8 || uintptr_t(p.bits) % 16))
    return fail(CLG_E_INVALID_ARG, "desc must be aligned to 8 bytes and bits to 16");
  return CLG_OK;
}
int ppay_pos_check(const uint64_t* pos, uint32_t kind) {
  if (!mem_kind_ok(kind)) return fail(CLG_E_INVALID_ARG, "pos: memory kind %u", kind);
  if (kind != CLG_MEM_HOST && uintptr_t(pos) % 8) return fail(CLG_E_INVALID_ARG, "pos must be aligned to 8 bytes");
  return CLG_OK;
}
// The scratch of either direction for n rows in nt tiles.
int ppay_work(clg_engine* e, uint64_t n, uint64_t nt, clg::PpayWork* w, clg::PpayRes** res) {
  const uint64_t wb[5] = {n * 4, nt * sizeof(clg_pack_block), nt * 8, nt * 8, nt * 16};
  clg::Carve<5> c;
  CHK(carve(e->d_ppaywork, wb, &c));
  *w = clg::PpayWork{c.at<uint32_t>(0), c.at<clg_pack_block>(1), c.at<uint64_t>(2), c.at<uint64_t>(3), c.at<uint64_t>(4)};
  CHK(e->h_ppayres.ensure(sizeof(clg::PpayRes)));
  *res = e->h_ppayres.as<clg::PpayRes>();
  return CLG_OK;
}

}  // namespace

// The decode into engine scratch and the columns of what it produced, also in engine scratch;
// then the pack, the wide rows as they are and (var) the payload column of the same rows.
// Every size is known before anything is written to the caller.  wpk (the packed-wide decodes):
// the wide rows are delivered packed as well and no plain row is copied to the caller; `wide` then
// carries only sizes, and var may come without pos, which is the prefix sum of w_var_len.
int decode_columns_packed(clg_engine* e, const DecodeRun& run, uint32_t n, clg_columns* wide, clg_payloads* var,
                          clg_packed* out, const PaySpansOf& spans_of, clg_packed_wide* wpk) {
  if (wide->tag || wide->order || wide->timestamp || wide->rng || wide->buffer_built)
    return fail(CLG_E_INVALID_ARG, "the narrow column pointers of `wide` must be NULL: those columns are delivered packed");
  if (wpk)
    for (int i = clg::kColNarrowArrays; i < clg::kColArrays; ++i)
      if (clg::col_ptr(*wide, i)) return fail(CLG_E_INVALID_ARG, "every column pointer of `sizes` must be NULL: the wide rows are delivered packed");
  if (!mem_kind_ok(wide->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", wide->out_kind);
  CHK(pack_out_check(clg::pack_view(*out)));
  if (wpk) CHK(pack_out_check(clg::pack_view(*wpk)));
  clg::col_reset_result(wide);
  clg::pack_reset_result(out);
  if (wpk) clg::wpack_reset_result(wpk);
  if (var) clg::pay_reset_result(var);
  const bool no_pos = wpk && var && var->var && !var->pos;

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
  clg::Carve<5> sc;
  CHK(carve(e->d_packcol, cb, &sc));
  clg_columns full{};
  full.tag = keep.d.tag, full.order = sc.at<int8_t>(0);
  full.timestamp = sc.at<int64_t>(1), full.rng = sc.at<int32_t>(2);
  full.buffer_built = sc.at<int32_t>(3), full.w_v0 = sc.at<int64_t>(4);
  full.w_idx = keep.d.w_idx, full.w_rc = keep.d.w_rc, full.w_v1 = keep.d.w_v1, full.w_var_off = keep.d.w_var_off;
  full.w_var_len = keep.d.w_var_len, full.w_sub = keep.d.w_sub;
  full.cap_tag = nr, full.cap_order = tot[0], full.cap_timestamp = tot[1], full.cap_rng = tot[2];
  full.cap_buffer_built = tot[3], full.cap_wide = nw;
  full.out_kind = CLG_MEM_DEVICE;
  CHK(columnize_device(e, keep.d, nullptr, 0, &full));

  // every size, before anything is written to the caller
  const clg::PackSrc src{{full.tag, full.order, full.timestamp, full.rng, full.buffer_built}, {nr, tot[0], tot[1], tot[2], tot[3]}};
  clg::PackIn pin{};
  CHK(pack_prepare(src, out, &pin));
  const clg::WPackSrc wsrc{full.tag, full.w_idx, full.w_rc, full.w_v1, full.w_var_off, full.w_var_len, full.w_sub, full.w_v0, nr, nw};
  // a small batch: k_pack_small sizes, checks and writes both halves, once the other checks are made
  const bool small = pack_small_takes(e, *out) && (!wpk || wpack_small_takes(e, nw));
  if (!small) {
    CHK(pack_sizes(e, out, &pin));
    if (wpk) CHK(wpack_sizes(e, wsrc, wpk));
  }
  int ps = CLG_OK;
  std::vector<clg::PaySpan> spans;
  std::vector<uint32_t> segtab;
  const std::vector<uint64_t> row_base = wide_row_base(sb.data(), n);
  if (var) {
    ps = spans_of(spans, segtab);
    if (ps == CLG_OK) ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var, true);
  }
  const std::string pay_err = g_err;
  const int w0 = clg::kColNarrowArrays, w1 = clg::kColArrays;  // (the wide arrays: the table's last seven)
  bool wide_any = false, wide_short = false;
  for (int i = w0; i < w1; ++i) wide_any = wide_any || clg::col_ptr(*wide, i);
  for (int i = w0; i < w1; ++i) wide_short = wide_short || (wide_any && clg::col_array_cap(*wide, i) < nw);
  const clg::PackView pv = clg::pack_view(*out), wpv = wpk ? clg::pack_view(*wpk) : clg::PackView{};
  const char* pay_short = !var || ps != CLG_OK || clg::pay_sizes_only(*var) ? nullptr
                          : !no_pos                                         ? clg::pay_short(*var, var->n_rows, var->n_var)
                          : var->cap_var < var->n_var                       ? "var"
                                                                            : nullptr;
  const char *pk_short = nullptr, *wpk_short = nullptr;
  if (small) {
    // The one launch, last of the checks: it fills every size, and writes unless a check before it
    // failed (then it is held to its sizes) or one of its own does.
    PackSmallCall c;
    c.pin = &pin, c.nout = out;
    if (wpk && nw) c.wsrc = &wsrc, c.wout = wpk;
    c.hold = wide_short || pay_short;
    uint32_t short_cap = clg::kPackSmallShortNone;
    CHK(pack_small(e, c, &short_cap));  // (its own capacity error, when it was not held)
    const char* name = short_cap & 1 ? "bits" : "desc";
    if (short_cap < 2) pk_short = name;
    else if (short_cap < clg::kPackSmallShortNone) wpk_short = name;
  } else {
    pk_short = clg::pack_sizes_only(pv) ? nullptr : clg::pack_short(pv);
    wpk_short = wpk && !clg::pack_sizes_only(wpv) ? clg::pack_short(wpv) : nullptr;
  }
  if (wide_short) return fail(CLG_E_CAPACITY, "the wide rows' arrays are too small (rows %llu)", (unsigned long long)nw);
  if (pk_short) return pack_capacity_error(pv, "packed columns", pk_short);
  if (wpk_short) return pack_capacity_error(wpv, "packed wide rows", wpk_short);
  if (pay_short) return pay_too_small(pay_short, var->n_rows, var->n_var);

  // the writes
  if (!small && !clg::pack_sizes_only(pv)) CHK(pack_write(e, pin, out));
  if (!small && wpk && !clg::pack_sizes_only(wpv)) CHK(wpack_write(e, wpk));
  if (wide_any && nw) {
    for (int i = w0; i < w1; ++i)
      CHK(copy_caller(e, clg::col_ptr(*wide, i), clg::col_ptr(full, i), nw * clg::kColArray[i].width, hipMemcpyDefault,
                      wide->out_kind));
    CHK(e->sync());
  }
  if (var && ps == CLG_OK && !clg::pay_sizes_only(*var))
    ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var, false, no_pos);
  else if (ps != CLG_OK)
    g_err = pay_err;
  if (cs != CLG_OK) {
    g_err = col_err;
    return cs;
  }
  return ps;
}

extern "C" {

int clg_pack_columns(clg_engine* e, const clg_columns* in, clg_packed* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::pack_reset_result(out);
  CHK(pack_out_check(clg::pack_view(*out)));
  clg::PackSrc src = clg::pack_src(*in);
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    if (src.n[c] && !src.col[c]) return fail(CLG_E_INVALID_ARG, "null input array (stream %u)", c);
  if (!mem_kind_ok(in->out_kind)) return fail(CLG_E_INVALID_ARG, "the columns' out_kind %u", in->out_kind);
  PlaceSpec ins[clg::kPackStreams];
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    ins[c] = {src.col[c], src.n[c] * clg::pack_stream_bytes(c), clg::pack_stream_bytes(c)};
  clg::Placement pl;
  const int st = place_in(e, e->d_packin, ins, clg::kPackStreams, in->out_kind, PlacePolicy::stage_if_unresolved, "stream", &pl);
  if (st != CLG_OK) return clg::pack_layout(src.n, out), st;  // (a misaligned stream: the layout is filled, as pack_sizes fills it)
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) src.col[c] = pl.at<const void>(c);
  clg::PackIn pin{};
  CHK(pack_prepare(src, out, &pin));
  if (pack_small_takes(e, *out)) {
    PackSmallCall c;
    c.pin = &pin, c.nout = out;
    return pack_small(e, c);
  }
  CHK(pack_sizes(e, out, &pin));
  return pack_finish(clg::pack_view(*out), "packed columns", [&] { return pack_write(e, pin, out); });
}

int clg_pack_wide(clg_engine* e, const clg_columns* in, clg_packed_wide* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::wpack_reset_result(out);
  CHK(pack_out_check(clg::pack_view(*out)));
  if (!mem_kind_ok(in->out_kind)) return fail(CLG_E_INVALID_ARG, "the columns' out_kind %u", in->out_kind);
  const uint64_t nr = in->n_rec, nw = in->n_class[clg::kColWide];
  const PlaceSpec ins[8] = {{in->tag, nw ? nr : 0, 1},         {in->w_idx, nw * 4, 4},     {in->w_rc, nw * 4, 4}, {in->w_v1, nw * 8, 8},
                            {in->w_var_off, nw * 4, 4}, {in->w_var_len, nw * 4, 4}, {in->w_sub, nw, 1},    {in->w_v0, nw * 8, 8}};
  for (int i = 1; i < 8; ++i)
    if (nw && !ins[i].p) return fail(CLG_E_INVALID_ARG, "null input array (%d)", i);
  if (nw && !in->tag) return fail(CLG_E_INVALID_ARG, "null input array (tag)");
  clg::Placement pl;
  CHK(place_in(e, e->d_wpackin, ins, 8, in->out_kind, PlacePolicy::stage_if_unresolved, "wide", &pl));
  const clg::WPackSrc src{pl.at<const uint8_t>(0),  pl.at<const uint32_t>(1), pl.at<const int32_t>(2), pl.at<const int64_t>(3),
                          pl.at<const uint32_t>(4), pl.at<const uint32_t>(5), pl.at<const uint8_t>(6), pl.at<const int64_t>(7),
                          nr,                       nw};
  if (nw && wpack_small_takes(e, nw)) {
    PackSmallCall c;
    c.wsrc = &src, c.wout = out;
    return pack_small(e, c);
  }
  CHK(wpack_sizes(e, src, out));
  return pack_finish(clg::pack_view(*out), "packed wide rows", [&] { return wpack_write(e, out); });
}

int clg_pack_payloads(clg_engine* e, const uint8_t* var, const uint64_t* pos, uint64_t n_rows, uint32_t in_kind,
                      clg_packed_payloads* out) {
  ENGINE_GUARD(e);
  if (!out) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::ppay_reset_result(out);
  out->n_rows = n_rows;
  CHK(ppay_kind_check(*out, ""));
  CHK(ppay_pos_check(pos, in_kind));
  if (!n_rows) return CLG_OK;  // nothing to launch
  if (!pos) return fail(CLG_E_INVALID_ARG, "null pos");
  const uint64_t nt = clg::ppay_blocks(n_rows);
  if (nt >> 31) return fail(CLG_E_INVALID_ARG, "%llu rows in one call", (unsigned long long)n_rows);
  // How many bytes of var there are is pos's last entry.  Host-readable input is checked here,
  // before that entry sizes a copy; device input is checked by the kernel, which reads no byte
  // of var at or past that entry, and a null var must not have any.
  uint64_t claim = 0;
  if (in_kind != CLG_MEM_DEVICE) {
    for (uint64_t k = 0; k < n_rows; ++k)
      if (clg::ppay_row_bad(k, pos[k], pos[k + 1])) {
        out->bad_row = k;
        return fail(CLG_E_INVALID_ARG, "packed payloads: row %llu of pos is not a row", (unsigned long long)k);
      }
    claim = pos[n_rows];
  } else if (!var) {
    CHK(e->h_ppayres.ensure(sizeof(clg::PpayRes)));
    HIPCHK(hipMemcpyAsync(e->h_ppayres.p, pos + n_rows, 8, hipMemcpyDeviceToHost, e->stream));
    CHK(e->sync());
    claim = *e->h_ppayres.as<uint64_t>();
  }
  if (claim && !var) return fail(CLG_E_INVALID_ARG, "null var");
  const PlaceSpec ins[2] = {{var, claim, 1}, {pos, (n_rows + 1) * 8, 8}};
  clg::Placement pin;
  CHK(place_in(e, e->d_ppayin, ins, 2, in_kind, PlacePolicy::stage_if_unresolved, "payload", &pin));
  const uint8_t* d_var = pin.at<const uint8_t>(0);
  const uint64_t* d_pos = pin.at<const uint64_t>(1);
  clg::PpayWork w;
  clg::PpayRes* res;
  CHK(ppay_work(e, n_rows, nt, &w, &res));
  // (bytes: pos, both rows of a pair at most, the lcps and a descriptor a tile)
  CHK(e->timed("pack_payloads", n_rows * 12 + 2 * claim + nt * 56,
               [&] { return clg::launch_ppay_lcp_scan(d_var, d_pos, n_rows, uint32_t(nt), w, res, e->stream); }));
  CHK(e->sync());
  if (res->bad_row != clg::kPpayNoRow) {
    out->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "packed payloads: row %llu of pos is not a row", (unsigned long long)res->bad_row);
  }
  out->n_var = res->n_var, out->n_bits = res->n_bits, out->n_tail = res->n_tail;
  if (clg::ppay_sizes_only(*out)) return CLG_OK;
  if (const char* name = clg::ppay_short(*out))
    return fail(CLG_E_CAPACITY, "packed payloads: %s is too small (blocks %llu, payload bytes %llu, tail bytes %llu)", name,
                (unsigned long long)nt, (unsigned long long)out->n_bits, (unsigned long long)out->n_tail);
  const PlaceSpec dst[3] = {{out->desc, nt * sizeof(clg_pack_block), 8}, {out->bits, out->n_bits, 16}, {out->tail, out->n_tail, 1}};
  clg::Placement pl;
  CHK(place_out(e->d_ppayout, dst, 3, out->out_kind, PlacePolicy::stage_if_unresolved, "packed payload", &pl));
  CHK(e->timed("pack_payloads", n_rows * 12 + nt * 64 + out->n_bits + 2 * out->n_tail, [&] {
    return clg::launch_ppay_write(d_var, d_pos, n_rows, uint32_t(nt), w, pl.at<clg_pack_block>(0), pl.at<uint8_t>(1),
                                  pl.at<uint8_t>(2), out->n_bits, out->n_tail, e->stream);
  }));
  CHK(stage_out(e, dst, 3, pl));
  return e->sync();
}

int clg_pack_payloads_host(const uint8_t* var, const uint64_t* pos, uint64_t n_rows, clg_packed_payloads* out) {
  const char* what = "";
  const int st = clg::ppay_build_host(var, pos, n_rows, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "packed payloads: %s", what);
}

int clg_unpack_payloads(clg_engine* e, const clg_packed_payloads* in, const uint64_t* pos, uint32_t pos_kind,
                        clg_payloads* out, clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  bool done;
  const char* what = "";
  const int st = clg::ppay_unpack_begin(in, pos, out, bad, &done, &what);
  if (st != CLG_OK) return fail(st, "unpack payloads: %s", what);
  if (done) return CLG_OK;
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  CHK(ppay_kind_check(*in, "the packed input's "));
  CHK(ppay_pos_check(pos, pos_kind));
  const auto finding = [&](uint32_t kind, uint64_t block, const char* text) {
    clg::pack_bad_set(bad, kind, CLG_PPAY_STREAM, block);
    return fail(CLG_E_INVALID_ARG, "unpack payloads: %s (block %llu)", text, (unsigned long long)block);
  };
  const char* const totals = "the tails do not sum to n_tail, or pos does not end at n_var";
  const uint64_t n = in->n_rows, nt = clg::ppay_blocks(n);
  if (!n) return in->n_tail || in->n_var ? finding(CLG_UNPACK_BAD_TOTAL, 0, totals) : CLG_OK;  // nothing to launch
  if (nt >> 31) return fail(CLG_E_INVALID_ARG, "%llu rows in one call", (unsigned long long)n);
  const PlaceSpec ins[3] = {{in->desc, nt * sizeof(clg_pack_block), 8}, {in->bits, in->n_bits, 16}, {in->tail, in->n_tail, 1}};
  const PlaceSpec pin[1] = {{pos, (n + 1) * 8, 8}};
  const PlaceSpec dst[1] = {{out->var, in->n_var, 1}};
  clg::Placement pl_in, pl_pos, pl_out;
  CHK(place_in(e, e->d_ppayin, ins, 3, in->out_kind, PlacePolicy::stage_if_unresolved, "packed payload input", &pl_in));
  CHK(place_in(e, e->d_ppaypos, pin, 1, pos_kind, PlacePolicy::stage_if_unresolved, "pos", &pl_pos));
  CHK(place_out(e->d_ppayout, dst, 1, out->out_kind, PlacePolicy::stage_if_unresolved, "var", &pl_out));
  const uint64_t* d_pos = pl_pos.at<const uint64_t>(0);
  clg::PpayWork w;
  clg::PpayRes* res;
  CHK(ppay_work(e, n, nt, &w, &res));
  // (bytes: a descriptor and its payload, pos, the lcps written)
  CHK(e->timed("unpack_payloads", nt * 56 + in->n_bits + n * 12, [&] {
    return clg::launch_ppay_in_scan(pl_in.at<const clg_pack_block>(0), pl_in.at<const uint8_t>(1), in->n_bits, d_pos, n,
                                    uint32_t(nt), w, res, e->stream);
  }));
  CHK(e->sync());
  if (res->bad_block != clg::kPpayNoRow) return finding(CLG_UNPACK_BAD_BLOCK, res->bad_block, "malformed block descriptor");
  if (res->bad_value != clg::kPpayNoRow)
    return finding(CLG_UNPACK_BAD_VALUE, res->bad_value, "an lcp or a length breaks the format's rules");
  if (res->n_tail != in->n_tail || res->n_var != in->n_var) return finding(CLG_UNPACK_BAD_TOTAL, 0, totals);
  CHK(e->timed("unpack_payloads", n * 12 + nt * 8 + in->n_tail + 2 * in->n_var, [&] {
    return clg::launch_ppay_out(pl_in.at<const uint8_t>(2), d_pos, n, uint32_t(nt), w, pl_out.at<uint8_t>(0), in->n_tail,
                                in->n_var, e->stream);
  }));
  CHK(stage_out(e, dst, 1, pl_out));
  return e->sync();
}

int clg_unpack_payloads_host(const clg_packed_payloads* in, const uint64_t* pos, clg_payloads* out, clg_unpack_bad* bad) {
  const char* what = "";
  const int st = clg::ppay_unpack_host(in, pos, out, bad, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack payloads: %s", what);
}

int clg_pack_wide_host(const clg_columns* in, clg_packed_wide* out) {
  const char* what = "";
  const int st = clg::wpack_build_host(in, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "packed wide rows: %s", what);
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

int clg_decode_logs_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                        clg_columns* sizes, clg_payloads* var, clg_packed* narrow, clg_packed_wide* wide) {
  ENGINE_GUARD(e);
  if (!sizes || !narrow || !wide || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_logs(e, log, start_epoch, n);
  return decode_columns_packed(e, src.run, n, sizes, var, narrow, src.spans_of, wide);
}

int clg_decode_host_columns_packed_wide(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                        const uint64_t* span_len, uint32_t n, clg_columns* sizes, clg_payloads* var,
                                        clg_packed* narrow, clg_packed_wide* wide) {
  ENGINE_GUARD(e);
  if (!sizes || !narrow || !wide || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_host(e, bytes, span_off, span_len, n);
  return decode_columns_packed(e, src.run, n, sizes, var, narrow, src.spans_of, wide);
}

int clg_pack_columns_host(const clg_columns* in, clg_packed* out) {
  const char* what = "";
  const int st = clg::pack_build_host(in, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "packed columns: %s", what);
}

}  // extern "C"
