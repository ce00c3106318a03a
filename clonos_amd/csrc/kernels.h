// kernels.h -- descriptors shared by the host engine (engine*.cpp) and the gfx950
// kernels (kernels.hip).  Plain structs, no HIP types.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "slice_order.h"

struct clg_digest;  // include/clonos_engine.h
struct clg_diff;
struct clg_pack_block;

namespace clg {

// ---- decode geometry ---------------------------------------------------------
// A tile is one wave's unit of decode work: a contiguous run of at most kTile bytes
// of one span, lying inside one HBM segment (or one 16 KiB window of a host-input
// staging buffer).  The tile is split into kRegions regions of kRegion bytes; each
// lane owns one region.  Coordinates inside a tile are "aligned coordinates":
// a = delta + (byte offset from the tile's first valid byte), so that abase + a is
// the byte's address and abase is 16-byte aligned.
constexpr int kRegion = 256;
constexpr int kRegions = 64;
constexpr int kTile = kRegion * kRegions;  // 16384
constexpr int kEntries = 64;               // transfer-table domain per region / per tile

struct TileDesc {
  const uint8_t* abase;  // 16-byte aligned
  uint32_t delta;        // first valid byte is abase[delta]  (delta < 16)
  uint32_t len;          // valid bytes (delta + len <= kTile)
  uint32_t span;         // owning span
  uint32_t pad;
  uint64_t span_off;     // span offset of abase[delta]
};

struct SpanDesc {
  uint32_t first_tile;
  uint32_t n_tiles;
  uint64_t len;
};

// Per-tile aggregate over tile entries e in [0, kEntries): e is the span offset of the
// first record start at/after the tile start, relative to the tile start.
// Packed u64: exit (u32, relative to the tile end; kExitErr / kExitFar sentinels) |
// cnt (u16) << 32 | wcnt (u16) << 48.
constexpr uint32_t kExitErr = 0xFFFFFFFFu;
constexpr uint32_t kExitFar = 0xFFFFFFFEu;

// Per-tile convergence info produced by the table kernel:
//   conv_entry[l]: entry offset of region l (relative to the region's first valid byte)
//                  shared by every live candidate path, or 0xFFFF if unknown;
//   conv_suffix[l]: records (low 16) and wide records (high 16) on that shared path
//                   from region l to the tile end.
struct TileConv {
  uint16_t entry[kRegions];
  uint32_t suffix[kRegions];
  uint32_t exit;       // tile exit (relative to tile end) of the shared path, or kExitErr
  uint32_t valid;      // 1 if any region converged
};

// Resolution output per tile (filled by the resolve kernel).
struct TileRes {
  uint32_t entry;      // tile-relative offset of the first record start (>= len: none)
  uint32_t limit;      // aligned coordinate where emission stops (failing record), or ~0
  uint32_t flags;      // kResTableLive: entry < kEntries and its table path is live
  uint32_t pad;
  uint64_t rec_base;   // record index of the tile's first record (span-relative)
  uint64_t wide_base;  // side-table index of the tile's first wide record (span-relative)
};
constexpr uint32_t kResTableLive = 1;

struct SpanRes {
  uint64_t n_rec;
  uint64_t n_wide;
  int32_t status;      // CLG_OK or decode error code
  int32_t err_tag;
  int64_t err_off;     // span offset of failing record
  uint64_t rec_base;   // exclusive prefix over spans (filled by the span-scan kernel)
  uint64_t wide_base;
};

struct DecodeOut {
  uint32_t* off;
  uint8_t* tag;
  int64_t* v0;
  uint32_t* w_idx;
  int32_t* w_rc;
  int64_t* w_v1;
  uint32_t* w_var_off;
  uint32_t* w_var_len;
  uint8_t* w_sub;
  uint64_t cap;
  uint64_t wcap;
};

// ---- fast decode: convergence points (decode_fast.hip) ----------------------------
// Fast-pipeline geometry: a tile's aligned coordinates [0, kTile) are split into kFOwn
// regions of kFRegion bytes (the last one takes the remainder).  Lane l < kFOwn owns
// region l; lanes kFOwn..63 compute the points of the span's NEXT tile's first kFNext
// regions (the same deterministic function that tile evaluates for itself), so a tile
// knows where its last segment must land without waiting for its neighbour.
constexpr uint32_t kFRegion = 268;  // 67 dwords: odd, so lane-strided LDS scans are conflict-free
constexpr int kFOwn = 61;
constexpr int kFNext = 3;
constexpr int kFPoints = kFOwn + kFNext;  // 64 = one wave
//
// conv[t * 64 + l] = aligned coordinate (tile t) of point l after filtering: a point is
// kept iff its candidates converged, it lies inside its tile, and it exceeds every earlier
// kept point of the same tile; kConvUnknown otherwise.
constexpr uint32_t kConvUnknown = 0xFFFFFFFFu;

// Per-lane segment [conv[l], conv[end]) parsed by k_fast_scan.  end in l+1..63 (>= kFOwn:
// a point of the next tile); kEndFail = parse failed or no point reached.
struct LaneSeg {
  uint8_t end;
  uint8_t flags;
  uint16_t far;   // end == kEndFar: the chain's next record start, bytes past the tile end
  uint32_t cnt;
  uint32_t wcnt;
};
constexpr uint8_t kEndFail = 0xFF;
// The segment passed every next-tile point (all three off the chain: a long record across
// the next tile's first region starts) and stops at a record start in the next tile instead;
// the resolve walks the next tile from there to one of its own points.
constexpr uint8_t kEndFar = 0xFE;

// Tile summary assuming the tile's entry is its first kept point f.
struct TileSum {
  uint32_t cnt, wcnt;
  uint8_t f;      // first kept own point (kEndFail: none)
  uint8_t x;      // exit: next tile's point index (0..kFNext-1) the chain lands on; kEndFail = none;
                  // kEndFar: a record start `far` bytes past the tile end
  uint16_t far;
  uint32_t pad2;
  uint64_t valid; // own lanes on the chain from f
};

struct FastRes {
  uint64_t valid;      // lanes whose segments are on the resolved path
  uint64_t rec_base;   // span-relative
  uint64_t wide_base;
};

// Device scratch the Serializable stream walker (jser_device.h) spills its handle, class
// descriptor, field and frame tables to once a stream outgrows the walker's private
// first tier.  Bump-allocated (*used reset before each decode); a walk that finds it
// full reports kJsSpill and the engine grows the arena and decodes again, so no table
// bound ever rejects a valid stream.
struct JArena {
  uint8_t* base;
  uint64_t cap;
  unsigned long long* used;
};

#ifndef CLG_FCANDS
#define CLG_FCANDS 32
#endif
constexpr int kCands = CLG_FCANDS;  // candidate entries per region (covers every fixed-layout record; <= 64)
constexpr int kJserCap = 256;  // Serializable stream-length table entries per tile

// Serializable candidates recorded where the log bytes are written (k_scatter), so the
// decode need not read the whole log to find them.  Per pool segment: hdr[s] = life << 32 |
// entries, and ent[s * cap + i] = position in the segment (low 16 bits) | code << 16, code the
// record length of the "03 AC ED 00 05" stream there (TC_STRING and flat objects that end
// inside the request's written bytes, strings well-formed) or kSideUnknown (another shape, a
// stream running past the request, or a prefix of the magic at its end: the decode verifies
// the magic and walks the stream).  A stream running past its chunk is measured on the
// request's next chunks' bytes (contiguous in the source) when the chunk says it goes on.
// `life` is the host's count of the segment's allocations (31 bits).  The chunk at a
// segment's offset 0 -- every life's first, segments filling from their start -- stamps it,
// resetting the list; a later chunk of that life with no candidate touches nothing.
// entries > cap: the list overflowed, the decode scans the segment's tiles.  Segments of
// more than 64 KiB carry no sidecar (hdr null).
constexpr uint32_t kSideUnknown = 0xFFFFu;
constexpr uint32_t kSideCapMax = 1024;  // entries per segment at most (C / 64, 64 KiB segments)
struct SideCar {
  uint64_t* hdr;
  uint32_t* ent;
  const uint8_t* pool;  // the segment pool (a tile outside it is scanned)
  uint64_t pool_bytes;
  uint32_t seg_bytes;
  uint32_t cap;
};

// Serializable stream lengths per tile, sorted by position (aligned coordinates):
// pos/len[t * kJserCap + i], n[t] entries (n > kJserCap: overflow, span falls back);
// defer[t] = 1 if the tile's scan met a "03 AC ED 00 05" pattern before the tables existed.
struct JserTabs {
  uint32_t* pos;
  uint32_t* len;
  uint32_t* n;
  uint32_t* defer;
  JArena ar;
  uint64_t* prof = nullptr;  // developer diagnostics: 16 s_memtime stamps per tile (fill 0-7, emit 8-15)
  SideCar side{};            // the write path's candidates (k_jser_fill takes a tile's table from them)
};

// Fused convergence + segment pass.  mode 0: every tile (tiles meeting a Serializable
// record are deferred); mode 1: only deferred tiles, stream-length tables filled.
int launch_fast_scan(const TileDesc* d_tiles, uint32_t n_tiles, const SpanDesc* d_spans, uint32_t* d_conv, JserTabs J,
                     uint32_t mode, LaneSeg* d_lanes, TileSum* d_sums, uint32_t* d_dbg, uint64_t* d_prof, void* stream);
int launch_jser_fill(const TileDesc* d_tiles, uint32_t n_tiles, const SpanDesc* d_spans, JserTabs J, void* stream);
int launch_fast_resolve(const TileDesc* d_tiles, const SpanDesc* d_spans, uint32_t n_spans, uint32_t* d_conv,
                        LaneSeg* d_lanes, const TileSum* d_sums, JserTabs J, FastRes* d_fres, SpanRes* d_sres,
                        uint32_t* d_span_flags, JArena ar, void* stream);
int launch_fast_emit(const TileDesc* d_tiles, uint32_t n_tiles, const SpanDesc* d_spans, const uint32_t* d_conv,
                     JserTabs J, const LaneSeg* d_lanes, const FastRes* d_fres, const SpanRes* d_sres,
                     const uint32_t* d_span_flags, DecodeOut out, void* stream);

// ---- fast decode (decode_fused.hip) -------------------------------------------------
// Three passes over tiles of kZTile bytes (64 regions of kZRegion bytes, one per lane):
// count (persistent grid, record chain + per-tile counts + record-start bitmaps), scan
// (record / wide bases per tile and per span), emit (SoA).  Any anomaly raises *abort and
// the host re-decodes the batch with the robust pipeline above.
constexpr uint32_t kZRegion = 128;
constexpr uint32_t kZTile = 64 * kZRegion;  // 8192
constexpr uint32_t kZHalo = 64;             // bytes of the span's next tile staged after a tile

// ---- the words the fused decode's kernels and the host exchange ----------------------
// FusedCtl::abort[k].  kZAbortAny is a flag, nonzero once any tile aborted (polled by waiting
// tiles); each reason's word holds ~(the lowest tile that aborted for it), 0 while none did;
// kZAbortJserSeen is a flag again.  As a value (count_tile's result) kZAbortNone: no abort.
enum ZAbort : uint32_t {
  kZAbortNone = 0,
  kZAbortAny = 0,
  kZAbortBad = 1,           // an invalid record on the true chain
  kZAbortEnd = 2,           // a span's last record does not end at the span end
  kZAbortExit = 3,          // a tile's exit is not the entry its successor took
  kZAbortTimeout = 4,       // a wait timed out
  kZAbortSerializable = 5,  // a Serializable record met without tables (the host runs again with them)
  kZAbortOverflow = 6,      // a Serializable table arena or work list full (the host grows it and runs again)
  kZAbortJserSeen = 7,      // phase 3 found Serializable candidates (any tile): the host keeps building tables
};
constexpr uint32_t kZAbortFlagWords = 8;
// The host's stat per reason (a count of aborted runs that met it).
constexpr const char* kZAbortStat[kZAbortFlagWords] = {
    nullptr,                 // kZAbortAny
    "decode_abort_bad",      // kZAbortBad
    "decode_abort_end",      // kZAbortEnd
    "decode_abort_exit",     // kZAbortExit
    "decode_abort_timeout",  // kZAbortTimeout
    "decode_abort_serializable",  // kZAbortSerializable
    "decode_abort_overflow",      // kZAbortOverflow
    nullptr,                 // kZAbortJserSeen
};
// FusedCtl::rep[k], the repair and check counters (zeroed per batch with the abort words).
enum ZRep : uint32_t {
  kZRepServed = 0,      // chunks walked again for a wrong entry (k_decode_repair)
  kZRepFiled = 1,       // repair requests the count pass filed
  kZRepLookback = 2,    // look-back checks failed (k_decode_emit; the batch is decoded again)
  kZRepCanonEarly = 3,  // canonical exits found before their tile's end (published as the tile end)
};
constexpr uint32_t kZRepWords = 4;
// abort[] and rep[] are one run of u32 words on the device (rep = abort + kZAbortFlagWords) and
// in the host's read-back (`hab` in the kernels and finish_fused): counter k is hab[zhab_rep(k)].
constexpr uint32_t kZAbortWords = kZAbortFlagWords + kZRepWords;
constexpr uint32_t zhab_rep(ZRep k) { return kZAbortFlagWords + k; }
// FusedCtl::jwork's header, then the work list ([kZJWorkHead, + cap) the items' table slots,
// the next cap words their tiles).  The header follows the abort words in the read-back.
enum ZJWork : uint32_t {
  kZJWorkItems = 0,  // items filed (past jwork_cap: the list was full)
  kZJWorkOvf = 1,    // overflow-arena entries taken (past jovf_cap: the arena was full)
};
constexpr uint32_t kZJWorkHead = 2;
constexpr uint32_t kZHabJWork = kZAbortWords;
static_assert(kZAbortFlagWords % 2 == 0 && kZAbortWords % 2 == 0 && kZJWorkHead % 2 == 0,
              "the u32 word groups start and end on the u64 words the layouts below count in");
// FusedCtl::dbg (CLONOS_FUSED_DEBUG), u32 words: the head, a record of kZDbgLaneWords words per
// lane of the first aborting tile from kZDbgLanes (rs, re, speculative exit / bad / first,
// 0, entry, exit | bad << 31), then from kZDbgTiles two u64 per tile: the entry its ex word
// was written from, and the writer.
enum ZDbg : uint32_t {
  kZDbgClaim = 0,  // the first aborting tile (count_tile claims the words up to kZDbgEndA and the lanes)
  kZDbgTile = 1,
  kZDbgReason = 2,
  kZDbgMustExit = 3,
  kZDbgXTrue = 4,
  kZDbgETrue = 5,
  kZDbgLo = 6,
  kZDbgHi = 7,
  kZDbgEndA = 8,
  kZDbgWalkMark = 9,  // kZDbgWalkGaveUp: a repair walk gave up, and then
  kZDbgWalkFrom = 10,
  kZDbgWalkAt = 11,
  kZDbgWalkEntry = 12,
  kZDbgWalkExit = 13,
  kZDbgWalkSpan = 14,
  kZDbgWalkDisagree = 15,
  kZDbgSkipN = 16,  // chunk-entry reads not taken (published, but before their tile); the first one:
  kZDbgSkipTile = 17,
  kZDbgSkipWordLo = 18,
  kZDbgSkipWordHi = 19,
  kZDbgSkipOff = 20,
  kZDbgSkipPolls = 21,
};
constexpr uint32_t kZDbgLanes = 24;  // (the head: [0, kZDbgLanes))
constexpr uint32_t kZDbgWalkGaveUp = 0xD15A;
constexpr uint32_t kZDbgLaneWords = 8;
constexpr uint32_t kZDbgTiles = kZDbgLanes + 64 * kZDbgLaneWords;  // the per-tile words' start (u32 index)

struct FusedCtl {
  uint64_t* st_x;     // per tile: pk_word(2, exit (span offset) the successor enters at)
  uint64_t* cnt;      // per tile: wide<<31 | records
  uint64_t* base;     // per tile: exclusive prefix of cnt inside its block of 1024 tiles
  uint64_t* boff;     // per block of 1024 tiles: exclusive prefix of the block totals
  uint64_t* bits;     // per tile: 64 x 16 B record-start bitmaps (lane l: region l)
  uint64_t* span_lo;  // per span: base at its first tile
  uint64_t* span_hi;  // per span: base past its last tile
  uint32_t* abort;    // [kZAbortFlagWords]: the batch's flag and ~(first tile) per abort reason (ZAbort)
  uint32_t* dbg;      // optional diagnostics (CLONOS_FUSED_DEBUG): the words of ZDbg
  uint64_t* prof;     // optional per-tile phase stamps (CLONOS_SCAN_PHASES): s_memtime x 8
  uint32_t n_tiles;
  // Serializable record lengths per tile (phase 3, k_decode_jser), sorted by position:
  // jpos/jlen[t * kZJCap + i] (aligned coordinate, record length or 0 for an invalid
  // stream), jn[t] entries.  jser = 1: the tables exist and the passes use them.
  uint32_t* jpos;
  uint32_t* jlen;
  uint32_t* jn;
  uint32_t jser;
  uint32_t jwork_cap;  // capacity of the general-walker work list
  uint32_t* jwork;     // the header (ZJWork), then cap words of the items' table slots, cap words of
                       // their tiles; with the sidecar then the count of tiles to scan and those
                       // tiles (n_tiles words)
  uint32_t warm;    // speculative warm-up bytes before each region (| 1 << 31: not staggered by lane)
  JArena jar;       // the stream walker's spill arena (k_decode_jser_general)
  // Per-span fallback: a tile whose chain goes wrong (kZAbortBad, End, Exit, Serializable) sets span_bad[span]
  // and the count pass goes on with the next span; the host decodes the bad spans with the
  // robust pipeline, injects their counts (k_decode_inject) and re-runs scan + emit with
  // skip_bad set, so emit leaves the bad spans' records to the robust output.
  uint32_t* span_bad;
  uint32_t skip_bad;
  // Count pass: block b's chunk is tiles [chunk[b], chunk[b + 1]) (chunks of about equal
  // bytes, decode_count_chunks), or null: equal tile counts.  A batch of many small spans
  // beside a few large ones (config 4: 320-byte subpartition logs, 22 KB main logs) would
  // otherwise give a few blocks chunks of only large tiles and make them the critical path.
  const uint32_t* chunk;
  uint32_t tiny;  // pass 0 ran (k_decode_count_tiny): small whole spans are counted already
  // Chunk-boundary repair (k_decode_count files, k_decode_repair serves): ex[t] = 1 << 63 |
  // the tile's exit (span offset), 0 while unknown; rep_flag[c] = 1: chunk c needs a check;
  // ent[c] = pk_word(2, the span offset chunk c's first tile entered at) when it entered at a
  // published exit (0: it did not).  k_decode_repair compares every such entry with the true
  // exit ex[] of the tile before, after the count pass, so a chunk that took a wrong entry is
  // walked again whatever the hand-off read returned.  rep[]: the counters of ZRep (a canonical
  // exit published as the tile end is a guess the repair checks).  All zeroed per batch.
  uint64_t* ex;
  uint8_t* rep_flag;
  uint32_t* rep;
  uint64_t* ent;
  // Test switch (CLONOS_FUSED_PERTURB): bits 15:0 are added to every chunk entry taken from a
  // published exit (and every small-path entry) -- the wrong entries the checks must catch;
  // bit 16 makes scan block 1's look-back result one record too high.  0 in production.
  uint32_t perturb;
  // 1: the one-launch scan (k_decode_scan) computed boff, and emit checks each block's
  // look-back result against its predecessor's final word (lb).  0: the three-launch scan.
  uint32_t lb_check;
  uint32_t n_spans;  // (the abort words' place in h_res)
  // Decode errors kept on the fast path: span_err[s] = the lowest span offset where a true
  // chain of span s met an invalid record (~0: none; atomicMin), and the tile holding it
  // writes the counts and start bits of the records before it.  null: off.
  uint64_t* span_err;
  // Serializable tables past kZJCap entries: entry i >= kZJCap of tile t at slot
  // n_tiles * kZJCap + jbase[t] + i - kZJCap of jpos / jlen (jovf_cap slots in all, taken
  // with jwork[kZJWorkOvf]; exhausted: kZAbortOverflow, the host grows the arena and runs again).
  uint32_t* jbase;
  uint32_t jovf_cap;
  // The one-launch scan (phase 5, k_decode_scan): lb[0] a ticket counter, lb[1 + b] block b's
  // look-back word (pk_word state 1 and its total, then state 2 and its inclusive prefix; the
  // state is held in both halves, see decode_fused.hip); all zeroed per
  // batch.  h_res: host memory the host reads the batch's result from (fused_readback below)
  // -- written by that kernel, so no read-back copy is queued (null: none).
  uint64_t* lb;
  uint64_t* h_res;
  uint32_t lean;  // batches without tables: the lean speculative walk (wide tags step one byte)
  // The write path's Serializable candidates (SideCar, below): phase 3 builds a tile's table
  // from its segment's list instead of scanning the tile (hdr null: every tile is scanned).
  SideCar side;
};
constexpr uint32_t kZScanBlock = 1024;  // tiles per workgroup of the offsets scan
static_assert(sizeof(FusedCtl) == 328, "the kernels' argument layout: no field added, resized or moved");

// The device control block of one batch (FusedCtl's pointers into it), in u64 words from its
// start.  This function alone knows the order
//   st_x[nt] ex[nt] rep_flag[nt] (u8) | cnt[nt] base[nt] boff[nb] | span_lo[ns] span_hi[ns] |
//   abort[kZAbortFlagWords] rep[kZRepWords] (u32) | lb: a ticket, look-back[nb] | ent[chunks]
// (nb blocks of kZScanBlock tiles, a chunk per block of the count pass's grid; bits lie apart).
// Three things rely on neighbours in it: the set-up zeroes [0, cnt) and [abort, words) as one
// range each (st_x, ex, rep_flag; the abort and repair words, lb, ent); rep is abort +
// kZAbortFlagWords; and span_lo | span_hi | abort | rep is the read-back's order, so a
// read-back is one copy from span_lo or from span_hi.
struct FusedLayout {
  size_t ex, rep_flag, cnt, base, boff, span_lo, span_hi, abort, lb, ent, words;  // (st_x: 0)
};
inline FusedLayout fused_layout(uint32_t n_tiles, uint32_t n_spans, uint32_t grid) {
  const size_t nt = n_tiles, ns = n_spans, nb = (nt + kZScanBlock - 1) / kZScanBlock;
  FusedLayout L;
  L.ex = nt;
  L.rep_flag = L.ex + nt;
  L.cnt = L.rep_flag + (nt + 7) / 8;
  L.base = L.cnt + nt;
  L.boff = L.base + nt;
  L.span_lo = L.boff + nb;
  L.span_hi = L.span_lo + ns;
  L.abort = L.span_hi + ns;
  L.lb = L.abort + kZAbortWords / 2;
  L.ent = L.lb + 1 + nb;
  L.words = L.ent + (grid ? grid : 1);
  return L;
}
// The host's read-back of a batch (h_zres, FusedCtl::h_res), in u64 words:
//   span_lo[ns] | span_hi[ns] | abort + rep (u32: `hab`) | the jwork header (u32, hab[kZHabJWork ..])
// The first three in the control block's order.  abort_only: up to the abort flag words (the
// per-span fallback's re-run reads no counters).
struct FusedReadback {
  uint32_t span_hi;
  uint64_t abort, abort_only, jwork, words;
};
constexpr FusedReadback fused_readback(uint32_t n_spans) {
  return FusedReadback{n_spans, 2ull * n_spans, 2ull * n_spans + kZAbortFlagWords / 2,
                       2ull * n_spans + kZHabJWork / 2, 2ull * n_spans + (kZHabJWork + kZJWorkHead) / 2};
}
constexpr uint32_t kZJCap = 256;  // Serializable candidates per tile in LDS (more: the overflow arena)
constexpr uint32_t kZTinySpan = 1024;   // whole spans up to this many bytes: pass 0, a lane each
// The launches of the fused decode (launch_decode_fused).  A batch takes Count, Scan, Emit in
// that order, after one optional launch: JserTables when it builds tables, or CountTiny when it
// holds small whole spans and builds none (the two never occur together).
// (Comments elsewhere name them by number: "phase 3" the tables, "phase 5" the one-launch scan,
// "pass 0" the small whole spans.)
enum class FusedPhase : uint32_t {
  Count = 0,       // count and chunk repair over a resident grid
  Scan3 = 1,       // the offsets in three launches, no look-back words (the per-span fallback's re-run)
  Emit = 2,        // the records out, a block per tile
  JserTables = 3,  // Serializable length tables (from the sidecar's lists where there are any)
  CountTiny = 4,   // small whole spans, a lane each
  Scan = 5,        // scan, block offsets and span ranges in one launch (ctl.lb zeroed)
};
// Per-span fallback: cnt[t] of every tile of bad span bad[i] := t == its first tile ?
// packed[i] (the robust decode's wide << 31 | records) : 0.
int launch_decode_inject(const SpanDesc* d_spans, const uint32_t* d_bad, const uint64_t* d_packed, uint32_t n_bad,
                         FusedCtl ctl, void* stream);
// x[i] += delta for i < n (the robust output's wide-row record indices moved into place).
int launch_add_u32(uint32_t* d_x, uint64_t n, uint32_t delta, void* stream);
// Per-span fallback, last step: bad span i's robust records (scratch rows [rbase, rbase + nrec),
// wide rows [wbase, wbase + nwide)) into the batch output at the span's bases from the re-run
// scan (ctl.span_lo), the wide rows' record indices moved by (batch base - rbase).
struct SfPlace {
  uint64_t rbase, nrec, wbase, nwide;
  uint32_t span, pad;
};
int launch_sf_place(const SfPlace* d_place, uint32_t n_bad, DecodeOut scratch, DecodeOut out, FusedCtl ctl, void* stream);
// Per-span fallback, first step (kernels.hip): bad span bad[i] with a recorded error position
// (ctl.span_err) -- the record there classified by decodeNext's full rules.  An invalid record
// (res[2 i] = its status < 0, res[2 i + 1] = its tag, as int8): the span keeps the fast run's
// records before it (span_bad cleared, its tiles past the error get no records).  Else (a
// valid record there: res[2 i] = 0) the span stays bad for the robust pipeline.
int launch_err_classify(const TileDesc* d_tiles, const SpanDesc* d_spans, const uint32_t* d_bad, uint32_t n_bad,
                        FusedCtl ctl, int32_t* d_res, JArena ar, void* stream);
int launch_decode_fused(const TileDesc* d_tiles, uint32_t n_tiles, const SpanDesc* d_spans, uint32_t n_spans,
                        FusedCtl ctl, DecodeOut out, void* stream, FusedPhase phase);
// The count pass's grid for n_tiles tiles (the blocks the device keeps resident, at most one
// per tile); CLG_E_DEVICE as 0.
uint32_t decode_count_grid(bool jser, uint32_t n_tiles);

// Small batches in one launch (k_decode_small_tiles): a block per tile counts the tile from
// its predecessor's published exit, publishes its own exit and counts, sums every earlier
// tile's (look-back), emits.  Batches without Serializable tables.  Results go to `res`
// (host-mapped pinned memory or device), the words of ZSmallRes.  agg: kZSmallAggWords zeroed
// words; the kernel zeroes all of agg_next for
// the next call (the host alternates two buffers, so no memset is queued).  plan (host memory,
// optional): a plan of at most kZSmallArgTiles tiles and kZSmallArgSpans spans goes in the
// launch's own arguments instead of d_tiles / d_spans, so no copy is queued before the launch.
constexpr uint32_t kZSmallSpans = 4096;     // spans per small batch at most
constexpr uint32_t kZSmallTilesMax = 4096;  // tiles per small batch at most
constexpr uint32_t kZSmallAggWords = 2 * kZSmallTilesMax;  // look-back words per buffer: counts, exits
constexpr uint32_t kZSmallArgTiles = 64, kZSmallArgSpans = 64;
enum ZSmallRes : uint32_t {
  kZSmallRec = 0,     // records
  kZSmallWide = 1,    // wide rows
  kZSmallFailed = 2,  // != 0 when any tile failed (the host then decodes the batch the usual way)
  kZSmallSpan0 = 3,   // [kZSmallSpan0 + s]: span s's first record (spans with tiles), then per tile
                      // the hand-offs it took, for the host's check: kZSmallCheckWords words
};
enum ZSmallCheck : uint32_t {
  kZCheckEntryExit = 0,  // entry | exit << 32 (span offsets; a small span is under 4 GiB)
  kZCheckBase = 1,       // the tile's base: every earlier tile's counts
  kZCheckCount = 2,      // its own counts (wide << 31 | records)
};
constexpr uint32_t kZSmallCheckWords = 3;
// Tile t's check words in `res` (host and device), and the words `res` holds in all.
constexpr uint64_t small_check_at(uint32_t n_spans, uint32_t t) {
  return uint64_t(kZSmallSpan0) + n_spans + uint64_t(kZSmallCheckWords) * t;
}
constexpr uint64_t small_res_words(uint32_t n_spans, uint32_t n_tiles) { return small_check_at(n_spans, n_tiles); }
struct SmallPlanArg {  // 3 KiB: with the other arguments inside the 4 KiB kernel-argument limit
  TileDesc tiles[kZSmallArgTiles];
  SpanDesc spans[kZSmallArgSpans];
};
int launch_decode_small(const TileDesc* d_tiles, uint32_t n_tiles, const SpanDesc* d_spans, uint32_t n_spans,
                        FusedCtl ctl, DecodeOut out, uint64_t* agg, uint64_t* agg_next, uint64_t* res, void* stream,
                        const SmallPlanArg* plan = nullptr);

// ---- gather (delta slice) -------------------------------------------------------
// A piece copies len bytes from src to out + dst; the source range lies inside one
// segment.  Pieces are produced per slice request and split at segment boundaries.
struct GatherPiece {
  const uint8_t* src;
  uint64_t dst;
  uint32_t len;
  uint32_t pad;
};

// ---- log digest (digest.h, digest.hip) ---------------------------------------------
// The constant table the digest kernels read, in u64 words: the square ladder R^(2^j), then
// R^(8 q) for q < 64 (a lane window is 8 words), R^k for k <= 8, and R^512 (a wave's words per
// iteration).  digest_table fills kDigestTabWords host words.
constexpr uint32_t kDigestTabWin = 32, kDigestTabOne = kDigestTabWin + 64, kDigestTabIter = kDigestTabOne + 9,
                   kDigestTabWords = kDigestTabIter + 1;
void digest_table(uint64_t* tab);
// Digest of each run: pass 1 writes one partial per piece (pieces as k_expand_pieces produces
// them: dst is the piece's offset in the packed order, runs[].dst its run's), pass 2 adds a
// run's partials and writes {hash, len} to d_out[run.pad].
int launch_digest(const GatherPiece* d_pieces, uint32_t n_pieces, const struct SegSpan* d_runs, uint32_t n_runs,
                  const uint64_t* d_tab, uint64_t* d_partial, ::clg_digest* d_out, void* stream);
// Prefix digests (digest.h): one cut of a request, in the order of the cuts.  dm: words the
// frame grows by from the cut before, m(cut) - m(previous cut); len: the cut clamped to the
// range; slot: the run (the non-empty stretch from the previous cut) whose sum S the cut adds,
// or kPrefixNoSlot for an empty stretch (S = 0).
struct PrefixCut {
  uint32_t dm, len, slot, pad;
};
constexpr uint32_t kPrefixNoSlot = 0xFFFFFFFFu;
// A chain of at most this many cuts per request everywhere in a call is walked by one thread.
constexpr uint32_t kPrefixFewCuts = 8;
// Digest of a range at each of its cuts: the runs are the non-empty stretches between cuts
// (d_lead[k]: run k's lead-in, its start in the range mod 4); pass 1 as launch_digest's in the
// range's word frame, pass 2 writes run k's sum to d_sums[k], pass 3 chains request i's cuts
// d_cuts[d_first[i] .. d_first[i + 1]) and writes a row per cut to d_out (few_cuts: every
// request has at most kPrefixFewCuts).
int launch_digest_prefixes(const GatherPiece* d_pieces, uint32_t n_pieces, const struct SegSpan* d_runs,
                           uint32_t n_runs, const uint32_t* d_lead, const uint64_t* d_first, uint32_t n_req,
                           const PrefixCut* d_cuts, bool few_cuts, const uint64_t* d_tab, uint64_t* d_partial,
                           uint64_t* d_sums, ::clg_digest* d_out, void* stream);

// ---- log comparison (diff.h, diff.hip) ---------------------------------------------
// The reference span of a run (parallel to the runs): its device address and length.
struct DiffRef {
  const uint8_t* ref;
  uint32_t len;
  uint32_t pad;
};
// Longest common prefix of each run and its reference span: pass 1 writes one u32 per piece
// (pieces as k_expand_pieces produces them), the offset in the piece of its first differing
// byte inside min(run, reference) or kDiffNone; pass 2 takes a run's minimum and writes
// {lcp, len_log, len_ref} to d_out[run.pad].
int launch_diff(const GatherPiece* d_pieces, uint32_t n_pieces, const struct SegSpan* d_runs, uint32_t n_runs,
                const DiffRef* d_refs, uint32_t* d_first, ::clg_diff* d_out, void* stream);

// ---- typed replay columns (columns.h, columns.hip) ---------------------------------
// Device addresses of a decoded batch's arrays and of the columns the kernels write.
struct ColIn {
  const uint8_t* tag;
  const int64_t* v0;
  const uint32_t* w_idx;
  uint64_t n, n_wide;
};
struct ColOut {
  int8_t* order;
  int64_t* timestamp;
  int32_t* rng;
  int32_t* buffer_built;
  int64_t* w_v0;
};
// The scan's results, in pinned memory the host reads: class totals, the first tile with a tag
// above 7 (kColNoTile: none); k_col_find_bad adds that tile's lowest such record and its tag.
constexpr uint64_t kColNoTile = ~0ull;
struct ColRes {
  uint64_t total[5];
  uint64_t bad_tile;
  uint64_t bad_index;
  uint64_t bad_tag;
};
// Count (a workgroup per tile -> d_counts[tile * kColCountWords]) and scan (one workgroup ->
// d_base[tile * 5], the exclusive per-class base of every tile; *res).
int launch_col_count_scan(const ColIn& in, uint32_t n_tiles, uint32_t* d_counts, uint64_t* d_base, ColRes* res,
                          void* stream);
// The lowest record of tile `tile` whose tag is above 7 -> res->bad_index / bad_tag (one wave).
int launch_col_find_bad(const ColIn& in, uint64_t tile, ColRes* res, void* stream);
// Write (a workgroup per tile; none without `write`), span bases (a wave per boundary:
// span_base[s * 5 + c] for s <= n_spans, from d_span_rec_base) and wide v0 (a thread per side
// row; none without out.w_v0).
int launch_col_write(const ColIn& in, uint32_t n_tiles, const uint64_t* d_base, const ColRes* res, bool write,
                     const ColOut& out, const uint64_t* d_span_rec_base, uint32_t n_spans, uint64_t* span_base,
                     void* stream);

// The one-launch form for small batches (k_col_small: one workgroup does count, scan, the
// check the host does for the multi-kernel form, write, span bases, wide v0 and the copies).
struct ColSmallIn {  // device addresses of the decoded batch; span_rec_base: pinned or device, null without spans
  const uint8_t* tag;
  const int64_t* v0;
  const uint32_t* w_idx;
  const int32_t* w_rc;
  const int64_t* w_v1;
  const uint32_t* w_var_off;
  const uint32_t* w_var_len;
  const uint8_t* w_sub;
  const uint64_t* span_rec_base;  // [n_spans + 1]
  uint64_t n, n_wide;
  uint32_t n_spans;
  uint32_t sizes_only;
};
// Where the columns go.  pack null: the twelve addresses as given (a null one is not written:
// the array is the input's own, or holds nothing).  pack set: the kernel lays all twelve out
// in pack, each section 16-byte aligned (col_pack_offsets), and the addresses are ignored.
struct ColSmallOut {
  uint8_t* tag;
  int8_t* order;
  int64_t* timestamp;
  int32_t* rng;
  int32_t* buffer_built;
  uint32_t* w_idx;
  int32_t* w_rc;
  int64_t* w_v1;
  uint32_t* w_var_off;
  uint32_t* w_var_len;
  uint8_t* w_sub;
  int64_t* w_v0;
  uint8_t* pack;
  uint64_t cap[6];  // usable capacities: tag, order, timestamp, rng, buffer_built, the wide rows
};
enum : uint32_t {
  kColSmallWritten = 0,   // the columns are written
  kColSmallSizes = 1,     // a sizes-only call: totals and span bases
  kColSmallBadTag = 2,    // bad_index / bad_tag
  kColSmallWideCount = 3, // n_wide differs from the wide total
  kColSmallCapacity = 4,  // short: the first short capacity's index in ColSmallOut::cap
};
struct ColSmallRes {  // pinned memory; with any verdict but kColSmallWritten no column is written
  uint64_t total[5];
  uint64_t bad_index;
  uint64_t bad_tag;
  uint32_t verdict;
  uint32_t short_cap;
  uint64_t pack_off[13];  // the packed sections' offsets in ColPtrs order; [12]: the end
};
// span_base: pinned, (n_spans + 1) * 5 entries, written with every verdict but kColSmallBadTag
// (null or n_spans 0: none).
int launch_col_small(const ColSmallIn& in, const ColSmallOut& out, ColSmallRes* res, uint64_t* span_base, void* stream);

// ---- the payload column (payload.h, payload.hip) -----------------------------------
// Where a span's bytes lie, one entry per span (empty spans included, so a row's span index is
// the entry's index).  base set: contiguous memory (a caller's device buffer, staged host
// input), span byte o at base[o].  base null: a range of a log in the segment pool, span byte o
// is physical byte p = phys + o, in segment segtab[segtab_off + p / C] at offset p % C
// (plan_log_span's rule: the table holds only the segments the span covers, phys rebased).
struct PaySpan {
  const uint8_t* base;
  uint64_t segtab_off;
  uint64_t len;
  uint32_t phys;
  uint32_t pad;
};
struct PayIn {  // device addresses
  const uint32_t* off;       // w_var_off[n_rows]
  const uint32_t* len;       // w_var_len[n_rows]
  const uint64_t* row_base;  // [n_spans + 1]
  const PaySpan* spans;      // [n_spans]
  const uint32_t* segtab;
  const uint8_t* pool;
  uint64_t n_rows;
  uint32_t n_spans;
  uint32_t seg_bytes;
};
// The scan's results, in pinned memory the host reads before anything is written to the caller.
struct PayRes {
  uint64_t n_var;
  uint64_t bad_row;  // kPayNoRow: none
};
// Size (a workgroup per tile of kPayTile rows -> d_sum[tile], d_bad[tile]) and scan (one
// workgroup -> d_base[tile], the bytes before the tile; *res).
int launch_pay_size_scan(const PayIn& in, uint32_t n_tiles, uint64_t* d_sum, uint64_t* d_bad, uint64_t* d_base,
                         PayRes* res, void* stream);
// Pos (pos[k] for k <= n_rows; none when pos is null) and copy (var; none when n_var is 0).  The
// copy scans its tile's lengths again and does not read pos, which may lie across the link.
int launch_pay_write(const PayIn& in, uint32_t n_tiles, const uint64_t* d_base, uint64_t n_var, uint64_t* pos,
                     uint8_t* var, void* stream);

// The one-launch form for small batches (k_pay_small: one workgroup does size, scan, the check
// the host does for the multi-kernel form, pos and the copy).
enum : uint32_t {
  kPaySmallWritten = 0,   // pos and var are written
  kPaySmallSizes = 1,     // a sizes-only call
  kPaySmallBadRow = 2,    // bad_row
  kPaySmallCapacity = 3,  // short: 0 pos, 1 var
};
struct PaySmallRes {  // pinned memory; with any verdict but kPaySmallWritten nothing is written
  uint64_t n_var;
  uint64_t bad_row;  // kPayNoRow: none
  uint32_t verdict;
  uint32_t short_cap;
};
// cap_pos / cap_var: usable capacities (0 for a null array).
int launch_pay_small(const PayIn& in, uint64_t* pos, uint8_t* var, uint64_t cap_pos, uint64_t cap_var, bool sizes_only,
                     PaySmallRes* res, void* stream);

// ---- packed typed columns (pack.h, pack.hip) ----------------------------------------
struct PackIn {  // device addresses of the five streams, their lengths and block bases
  const void* col[5];
  uint64_t n[5];
  uint64_t blk_base[6];
};
// The offset scan's total, in pinned memory the host reads before anything is written to the caller.
struct PackRes {
  uint64_t n_bits;
};
// Measure (a workgroup per block -> d_desc[block]: ref, first, width, count, and the payload's
// size in pos) and the offsets (group sums, one workgroup over the sums, then every group's
// scan plus its base: d_desc[block].pos becomes the payload's offset; *res the total).
// d_gsum: a u64 per group of kPackScanGroup blocks.
int launch_pack_measure_scan(const PackIn& in, uint32_t n_blocks, clg_pack_block* d_desc, uint64_t* d_gsum, PackRes* res,
                             void* stream);
// Write (a workgroup per block): descriptor b to out_desc[b] for b < lim_desc, its payload to
// bits + pos; no store at or past bits + lim_bits.
int launch_pack_write(const PackIn& in, uint32_t n_blocks, const clg_pack_block* d_desc, clg_pack_block* out_desc,
                      uint8_t* bits, uint64_t lim_desc, uint64_t lim_bits, void* stream);

// The offsets alone, over descriptors whose pos holds the payload's size (the three scan kernels
// know nothing of streams: pack_wide.hip's descriptors go through them too).
int launch_pack_scan(uint32_t n_blocks, clg_pack_block* d_desc, uint64_t* d_gsum, PackRes* res, void* stream);

// ---- packed wide rows (pack_wide.h, pack_wide.hip) ----------------------------------
struct WPackSrc {  // device addresses of the tags and the seven wide arrays
  const uint8_t* tag;
  const uint32_t* w_idx;
  const int32_t* w_rc;
  const int64_t* w_v1;
  const uint32_t* w_var_off;
  const uint32_t* w_var_len;
  const uint8_t* w_sub;
  const int64_t* w_v0;
  uint64_t n_rec, n_wide;
};
// The 26 streams' arrays, lengths and block bases.  It lives in device memory and is passed by
// address: the kernels index it with a wave-uniform stream number, which for a by-value kernel
// argument would go through scratch.
struct WPackTab {
  const void* col[26];
  uint64_t n[26];
  uint64_t blk_base[27];
};
constexpr uint32_t kWPackTile = 1024;  // rows a workgroup of the kind and split passes
// The scan's results, in pinned memory the host reads before it lays the streams out.
struct WPackRes {
  uint64_t tot[4];
  uint64_t bad_row;  // ~0: none
};
// Kind and count (a workgroup per tile: d_kind[row], d_cnt[tile * 4 + kind]; the lowest bad row
// into *d_bad by atomicMin, which this call first sets to ~0 through the stream) and the scan of
// the tile counts (one workgroup: d_base[tile * 4 + kind] the rows of that kind before the tile;
// *res).
int launch_wpack_count_scan(const WPackSrc& src, uint32_t n_tiles, uint8_t* d_kind, uint32_t* d_cnt, uint64_t* d_base,
                            unsigned long long* d_bad, WPackRes* res, void* stream);
// Split (a workgroup per tile: the six fields of every row to d_tab's per-kind arrays at the
// row's rank; no store at or past a kind's length) and measure (a workgroup per block of the 26
// streams -> d_desc[block] with the payload's size in pos; launch_pack_scan turns it into the offset).
int launch_wpack_split_measure(const WPackSrc& src, uint32_t n_tiles, const uint8_t* d_kind, const uint64_t* d_base,
                               const WPackTab* d_tab, uint32_t n_blocks, clg_pack_block* d_desc, void* stream);
// Write (a workgroup per block), as launch_pack_write.
int launch_wpack_write(const WPackTab* d_tab, uint32_t n_blocks, const clg_pack_block* d_desc, clg_pack_block* out_desc,
                       uint8_t* bits, uint64_t lim_desc, uint64_t lim_bits, void* stream);

// ---- both packs in one launch of one workgroup (pack.h, pack_wide.h, pack_small.hip) ------------
// A narrow input of at most kPackSmallBlocks blocks and at most kWPackSmallRows wide rows, either
// or both: every pass of the two multi-kernel forms and the host's checks between them.
struct PackSmallOut {  // one half's output and usable capacities (0 for a null array)
  clg_pack_block* desc;
  uint8_t* bits;  // packed: ignored, the payloads follow the descriptors at desc + blocks
  uint64_t cap_desc, cap_bits;
  uint32_t write;   // 0: this half is sizes only (or absent)
  uint32_t packed;  // engine staging, desc | bits in one piece
};
struct PackSmallArgs {
  PackIn narrow;   // n all zero: no narrow half
  WPackSrc wide;   // n_wide 0: no wide half
  uint8_t* d_kind;  // engine scratch: n_wide kind bytes, and the per-kind field arrays
  uint8_t* d_soa;   // (wpack_soa_field's layout, 16-byte aligned)
  PackSmallOut out_narrow, out_wide;
  uint32_t sizes_only;  // nothing is written, whatever the outputs say
};
enum : uint32_t {
  kPackSmallWritten = 0,   // every half with `write` set is written
  kPackSmallSizes = 1,     // sizes_only, or no half to write
  kPackSmallBadRow = 2,    // bad_row; no size of the wide half is filled
  kPackSmallCapacity = 3,  // short_cap
};
enum : uint32_t { kPackSmallShortNone = 4 };  // short_cap: 0 narrow desc, 1 narrow bits, 2 wide desc, 3 wide bits
struct PackSmallRes {  // pinned memory; with any verdict but kPackSmallWritten nothing is written
  uint64_t n_bits[2];  // narrow, wide
  uint64_t tot[4];     // the kinds' totals
  uint64_t bad_row;    // ~0: none
  uint32_t verdict;
  uint32_t short_cap;  // the first short capacity (also filled with kPackSmallSizes), or kPackSmallShortNone
};
int launch_pack_small(const PackSmallArgs& a, PackSmallRes* res, void* stream);

// ---- packed typed columns as input (pack.h, unpack.hip) -----------------------------
struct UnpackIn {  // device addresses of a clg_packed read as input, after the host's layout check
  const clg_pack_block* desc;
  const uint8_t* bits;
  uint64_t n[5];
  uint64_t blk_base[6];
  uint64_t n_bits;
};
struct UnpackOut {  // device addresses of the five plain columns, each aligned to its element
  void* col[5];
};
// The check's verdict: ~(the lowest bad block's index in desc) per kind, 0 when none.  Device
// memory that launch_unpack_check zeroes through the stream before the kernel's vector atomicMax
// (only a bad block issues one); copy it to the host after the kernel.
struct UnpackVerdict {
  unsigned long long bad_block;
  unsigned long long bad_value;
};
// Check (a wave per block, all five streams in one grid): the block check on every descriptor
// and, where the type does not already hold [ref, ref + 2^width - 1], every value.  No address
// is formed from a descriptor that failed the block check.
int launch_unpack_check(const UnpackIn& in, uint32_t n_blocks, UnpackVerdict* d_verdict, void* stream);
// Write (a workgroup per block), after a clean check: the plain values of every block to
// out.col[stream] + the block's first index.  A descriptor that fails the block check (the
// input changed under the call) writes nothing; no store at or past a stream's n.
int launch_unpack_write(const UnpackIn& in, const UnpackOut& out, uint32_t n_blocks, void* stream);

// ---- packed wide rows as input (pack_wide.h, unpack_wide.hip) -----------------------
// A clg_packed_wide read as input, after the host's layout check, and where its 26 streams'
// plain values go: col[0] the kind bytes and col[2 ..] the per-kind field arrays, all in engine
// scratch; col[1] w_idx of the rows (the caller's array or its scratch).  Device memory, passed by
// address, as WPackTab is.
struct WUnpackTab {
  const clg_pack_block* desc;
  const uint8_t* bits;
  uint64_t n_bits;
  uint64_t n[26];
  uint64_t blk_base[27];
  void* col[26];
};
// The rows in row order: the six field arrays in kWPackField's order (w_var_off may be null: not
// written), each aligned to its element.  tag (the combined calls: the narrow unpack's tags, n_rec
// of them) may be null: no cross rule.
struct WUnpackDst {
  void* col[6];
  const uint8_t* tag;
  uint64_t n_rec;
};
// The verdict words.  Device memory that launch_wunpack_check sets through the stream (the first
// two to 0, cross_row to ~0) before the kernels' vector atomicMax / atomicMin; only a finding
// issues one.  bad_block / bad_value: ~(the lowest bad block's index in desc).  cross_row: the
// lowest row whose w_idx names no wide record of its kind (raised by the merge).
struct WUnpackVerdict {
  unsigned long long bad_block;
  unsigned long long bad_value;
  unsigned long long cross_row;
};
// The scan's totals (KIND's histogram over the values 0 .. 3), in pinned memory.
struct WUnpackRes {
  uint64_t tot[4];
};
// Check (a wave per block, all 26 streams), kind (a workgroup per KIND block: d_tab->col[0] and
// d_cnt[tile * 4 + kind]) and the scan of the tile counts (one workgroup: d_base, *res).
int launch_wunpack_check(const WUnpackTab* d_tab, uint32_t n_blocks, uint32_t n_tiles, uint32_t* d_cnt, uint64_t* d_base,
                         WUnpackVerdict* d_verdict, WUnpackRes* res, void* stream);
// After a clean verdict.  Write (a workgroup per block of streams 1 .. 25, to d_tab->col), then
// merge (a workgroup per tile: the rows in row order to dst, the tile's sum of w_var_len to
// d_tsum), then, with pos, the scan of the tile sums and pos[0 .. n_wide].  No store at or past a
// stream's length or a row array's n_wide.
int launch_wunpack_write(const WUnpackTab* d_tab, uint32_t n_blocks, uint32_t n_kind_blocks, uint32_t n_tiles,
                         const uint64_t* d_base, const WUnpackDst& dst, uint64_t n_wide, uint64_t* d_tsum, uint64_t* pos,
                         WUnpackVerdict* d_verdict, void* stream);

// ---- the packed payload column (ppay.h, ppay.hip) -----------------------------------
// The pack's scratch: a row's lcp, a tile's descriptor (pos: the payload's size, then its offset),
// tail sum, tail base and lowest bad row.
struct PpayWork {
  uint32_t* lcp;
  clg_pack_block* desc;
  uint64_t* tsum;
  uint64_t* tbase;
  uint64_t* bad;  // the pack: a tile's lowest bad row; the unpack: [2 * tile] block, [2 * tile + 1] value finding
};
// The scans' results, in pinned memory the host reads before anything is written to the caller.
struct PpayRes {
  uint64_t n_tail;     // the sum of len - lcp
  uint64_t n_bits;     // the pack only
  uint64_t n_var;      // pos[n_rows] as the device read it
  uint64_t bad_row;    // the pack: the lowest bad row, ~0: none
  uint64_t bad_block;  // the unpack: the lowest tile that fails the block check, ~0: none
  uint64_t bad_value;  // ... the value rules
};
// The pack's lcp pass (a workgroup per tile: lcp, the tile's descriptor, tail sum and lowest bad
// row) and the scan (one workgroup: tail bases, the payloads' offsets, *res).  No byte of var at or
// past pos[n_rows] is read, and none of a tile that holds a bad row.
int launch_ppay_lcp_scan(const uint8_t* var, const uint64_t* pos, uint64_t n_rows, uint32_t n_tiles, const PpayWork& w,
                         PpayRes* res, void* stream);
// The pack's write, after the host's checks: the descriptors, the blocks' payloads below n_bits
// and the tails below n_tail.
int launch_ppay_write(const uint8_t* var, const uint64_t* pos, uint64_t n_rows, uint32_t n_tiles, const PpayWork& w,
                      clg_pack_block* desc, uint8_t* bits, uint8_t* tail, uint64_t n_bits, uint64_t n_tail, void* stream);
// The unpack's check (a workgroup per tile: the block check, the lcps, the pos and lcp rules, the
// tail sum) and the scan (one workgroup: tail bases, the lowest findings, *res).  No address is
// formed from a descriptor that failed the block check.
int launch_ppay_in_scan(const clg_pack_block* desc, const uint8_t* bits, uint64_t n_bits, const uint64_t* pos, uint64_t n_rows,
                        uint32_t n_tiles, const PpayWork& w, PpayRes* res, void* stream);
// The unpack's write, after a clean verdict: every row's prefix and tail to var + pos[k], below n_var.
int launch_ppay_out(const uint8_t* tail, const uint64_t* pos, uint64_t n_rows, uint32_t n_tiles, const PpayWork& w,
                    uint8_t* var, uint64_t n_tail, uint64_t n_var, void* stream);

// ---- append scatter ---------------------------------------------------------------
struct ScatterChunk {
  uint8_t* dst;        // inside one segment
  uint64_t src;        // offset into the staged upload buffer
  uint32_t len;
  uint32_t life;       // causal-log chunks: the segment's life stamp (SideCar, 31 bits) | 1 << 31:
                       // the request goes on in the next chunk, its source bytes contiguous
};

// ---- device-side planning ---------------------------------------------------------
// A run of a log's physical bytes.  Its gather pieces (one per segment it touches) or
// decode tiles (one per min(segment, kTile) window) are generated on the device from the
// log's segment-index table, uploaded once per call as one concatenated array, so host
// work per call is O(requests + logs), not O(segments).  (struct SegSpan: slice_order.h,
// with the order of a batched slice's runs.)
// Launch helpers' status: CLG_OK, or CLG_E_DEVICE with the HIP error kept (thread-local)
// for the engine's error text (take_launch_error, nullptr when none).
int launch_status(hipError_t e);
const char* take_launch_error();
int launch_expand_pieces(const SegSpan* d_spans, uint32_t n_spans, uint32_t n_pieces, const uint32_t* d_segtab,
                         const uint8_t* pool, uint32_t seg_bytes, GatherPiece* d_out, void* stream);
int launch_expand_tiles(const SegSpan* d_spans, uint32_t n_spans, uint32_t n_tiles, const uint32_t* d_segtab,
                        const uint8_t* pool, uint32_t seg_bytes, uint32_t unit, TileDesc* d_out, void* stream);
// The fast decode's set-up in one launch: n_tiles tiles expanded from the runs (as
// k_expand_tiles; 0: none), then each word range r[] copied from src or filled with val.
constexpr int kPrepRanges = 8;
struct PrepRange {
  uint32_t* dst;
  const uint32_t* src;  // null: fill
  uint64_t n;           // 32-bit words
  uint32_t val;
  uint32_t pad;
};
struct PrepArgs {
  const SegSpan* runs;
  uint32_t n_runs, n_tiles;
  const uint32_t* segtab;
  const uint8_t* pool;
  uint32_t C, U;
  TileDesc* tiles;
  uint64_t total;  // (set by the launcher)
  PrepRange r[kPrepRanges];
};
int launch_decode_prep(PrepArgs a, void* stream);

// ---- launchers (kernels.hip) -----------------------------------------------------------
// side: the causal pool's sidecar (null: no candidates recorded, e.g. in-flight log buffers)
int launch_scatter(const ScatterChunk* d_chunks, uint32_t n, const uint8_t* d_src, void* stream,
                   const SideCar* side = nullptr);
int launch_gather(const GatherPiece* d_pieces, uint32_t n, uint8_t* d_out, void* stream);
// Robust pipeline (per-byte DP transfer tables); runs only on spans whose flag is set
// (d_span_flags == nullptr: all spans).
int launch_decode_tables(const TileDesc* d_tiles, uint32_t n_tiles, const SpanDesc* d_spans,
                         uint64_t* d_agg, TileConv* d_conv, const uint32_t* d_span_flags, JArena ar, void* stream);
int launch_decode_resolve(const TileDesc* d_tiles, const SpanDesc* d_spans, uint32_t n_spans,
                          const uint64_t* d_agg, const TileConv* d_conv, TileRes* d_tres,
                          SpanRes* d_sres, const uint32_t* d_span_flags, JArena ar, void* stream);
int launch_decode_spanscan(SpanRes* d_sres, uint32_t n_spans, uint64_t* d_totals, void* stream);
int launch_decode_emit(const TileDesc* d_tiles, uint32_t n_tiles, const SpanDesc* d_spans,
                       const TileConv* d_conv, const TileRes* d_tres, const SpanRes* d_sres,
                       const uint32_t* d_span_flags, DecodeOut out, JArena ar, void* stream);


// ---- batched encode (encode.hip) -------------------------------------------------
struct EncodeIn {  // device pointers, the decode's SoA layout (clg_decoded)
  const uint8_t* tag;
  const int64_t* v0;
  const uint32_t* w_idx;
  const int32_t* w_rc;
  const int64_t* w_v1;
  const uint32_t* w_var_off;  // into var
  const uint32_t* w_var_len;
  const uint8_t* w_sub;
  const uint8_t* var;
  uint64_t n, n_wide;
  uint64_t var_len;  // bytes of var: a payload row's [w_var_off, + w_var_len) lies inside
};
// phase 0: wide prefix per block (wsum -> wbase, nb + 1), bytes per block (bsum -> bbase,
// nb + 1), *bad = lowest invalid record; phase 1: write.  nb = ceil(n / 1024).
int launch_encode(const EncodeIn& in, uint32_t* d_wsum, uint64_t* d_wbase, uint64_t* d_bsum, uint64_t* d_bbase,
                  uint32_t* d_bad, uint8_t* d_out, uint32_t phase, void* stream);

// ---- encode typed columns (encode_columns.h, encode_columns.hip) -----------------
struct EcolIn {  // device addresses of clg_columns_in's arrays (w_idx, pos, var: null when not given)
  const uint8_t* tag;
  const int8_t* order;
  const int64_t* timestamp;
  const int32_t* rng;
  const int32_t* buffer_built;
  const int32_t* w_rc;
  const int64_t* w_v1;
  const uint32_t* w_var_len;
  const uint8_t* w_sub;
  const int64_t* w_v0;
  const uint32_t* w_idx;
  const uint64_t* pos;
  const uint8_t* var;
  uint64_t n;
  uint64_t n_class[5];  // the stated column lengths: no column is indexed at or past them
  uint64_t n_var;
};
struct EcolRes {  // pinned memory: the byte scan's results
  uint64_t n_bytes;
  uint64_t bad_row;  // kEcolNone: none
};
// Bytes (a workgroup per tile of kEcolTile records -> d_sum[tile], d_bad[tile]), scan64 (one
// workgroup -> d_bbase[tile]; *eres) and span bases (a wave per boundary; none when d_span_base is
// null): span_out[s * 2] the byte base, [s * 2 + 1] 1 for a row that is not the tags' counts.
// d_base / cres: k_col_scan's per-tile class bases and totals over the same tags.
int launch_ecol_sizes(const EcolIn& in, uint32_t n_tiles, const uint64_t* d_base, uint64_t* d_sum, uint64_t* d_bad,
                      uint64_t* d_bbase, const ColRes* cres, EcolRes* eres, const uint64_t* d_span_base, uint32_t n_spans,
                      uint64_t* span_out, void* stream);
// Write (a workgroup per tile): no store at or past d_out + n_bytes.
int launch_ecol_write(const EcolIn& in, uint32_t n_tiles, const uint64_t* d_base, const uint64_t* d_bbase,
                      uint64_t n_bytes, uint8_t* d_out, void* stream);

// ---- replay preparation: subpartition recovery buffers ----------------------------
// A recovery buffer may hold BufferBuilt determinants only (ReplayingState.java:172-177),
// which are 5 bytes each, so record k of a well-formed buffer starts at 5k: no chain walk.
struct BufSpan {
  const uint8_t* src;  // device bytes
  uint64_t len;
  uint64_t out_base;   // first index in the sizes array
};
struct BufChunk {      // records [k0, k1) of span `span`
  uint32_t span;
  uint32_t pad;
  uint64_t k0, k1;
};
// first_bad[s] = lowest k whose record is not a complete BufferBuilt (init ~0).
int launch_bufsizes(const BufChunk* d_chunks, uint32_t n_chunks, const BufSpan* d_spans, int32_t* d_sizes,
                    uint64_t* d_first_bad, void* stream);
// Per span: the count of valid sizes, and the status SubpartitionRecoveryThread.run hits at
// record first_bad (decodeNext's error, or CLG_E_NOT_BUFFER_BUILT for a valid other record).
int launch_bufsizes_classify(const BufSpan* d_spans, uint32_t n_spans, const uint64_t* d_first_bad,
                             uint64_t* d_count, int32_t* d_status, int64_t* d_err_off, int32_t* d_err_tag,
                             JArena ar, void* stream);

}  // namespace clg
