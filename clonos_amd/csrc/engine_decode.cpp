// engine_decode.cpp -- decoding determinants: the plans and their staging, the fused
// three-pass decode, the one-launch decode of small batches, the per-span fallback, the
// asynchronous decodes and the robust pipeline, with the clg_decode_* entry points.
#include "engine_impl.h"

// Span filter of a plan (the per-span fallback re-decodes single spans): false = skip.
bool clg_engine::plan_keep(const DecodePlan& p, uint32_t* s) {
  if (!p.only) return true;
  const auto it = std::lower_bound(p.only->begin(), p.only->end(), *s);
  if (it == p.only->end() || *it != *s) return false;
  *s = uint32_t(it - p.only->begin());
  return true;
}

// Tile window for device planning: min(segment, tile) when one divides the other.
uint32_t clg_engine::tile_unit(uint32_t k) const {
  const uint32_t c = C();
  if (c <= k) return (k % c == 0) ? c : 0;
  return (c % k == 0) ? k : 0;
}

void clg_engine::plan_host_span(DecodePlan& p, const uint8_t* dbase, uint64_t len, uint32_t s, uint32_t T) {
  if (!plan_keep(p, &s)) return;
  clg::SpanDesc sd{uint32_t(p.tiles.size()), 0, len};
  uint64_t o = 0;
  while (o < len) {
    const uintptr_t addr = uintptr_t(dbase + o);
    const uint32_t delta = uint32_t(addr & 15);
    const uint32_t take = uint32_t(std::min<uint64_t>(len - o, uint64_t(T - delta)));
    p.tiles.push_back(clg::TileDesc{reinterpret_cast<const uint8_t*>(addr & ~uintptr_t(15)), delta, take, s, 0, o});
    o += take;
    sd.n_tiles++;
  }
  p.n_tiny += (sd.n_tiles == 1 && len <= clg::kZTinySpan) ? 1u : 0u;
  p.spans.push_back(sd);
  p.n_tiles = uint32_t(p.tiles.size());
}

void clg_engine::plan_log_span(DecodePlan& p, const Log& l, int32_t start, int32_t len, uint32_t s, uint32_t T) {
  if (!plan_keep(p, &s)) return;
  p.unit = tile_unit(T);
  if (const uint32_t U = p.unit) {  // device planning
    const uint32_t cnt = len > 0 ? (uint32_t(start + len - 1) / U - uint32_t(start) / U + 1) : 0;
    p.spans.push_back(clg::SpanDesc{p.n_tiles, cnt, uint64_t(len)});
    p.n_tiny += (cnt == 1 && uint32_t(len) <= clg::kZTinySpan) ? 1u : 0u;
    if (cnt) {  // only the segments the span covers go into the table (phys rebased on them)
      const uint32_t s0 = uint32_t(start) / C(), s1 = uint32_t(start + len - 1) / C() + 1;
      p.runs.push_back(clg::SegSpan{p.segtab.size(), uint32_t(start) - s0 * C(), uint32_t(len), s, p.n_tiles, 0});
      p.segtab.insert(p.segtab.end(), l.segs.begin() + s0, l.segs.begin() + s1);
    }
    p.n_tiles += cnt;
    return;
  }
  clg::SpanDesc sd{uint32_t(p.tiles.size()), 0, uint64_t(len)};
  int32_t ph = start;
  const int32_t end = start + len;
  while (ph < end) {
    const uint32_t si = uint32_t(ph) / C(), so = uint32_t(ph) % C();
    const uint32_t take = std::min<uint32_t>(uint32_t(end - ph), C() - so);
    // tiles never exceed kTile aligned bytes: split large segments
    uint32_t done = 0;
    while (done < take) {
      const uint32_t o = so + done;
      const uint32_t delta = o & 15;
      const uint32_t t = std::min<uint32_t>(take - done, T - delta);
      p.tiles.push_back(clg::TileDesc{seg_addr(l.segs[si]) + (o & ~15u), delta, t, s, 0, uint64_t(ph - start + int32_t(done))});
      done += t;
      sd.n_tiles++;
    }
    ph += int32_t(take);
  }
  p.n_tiny += (sd.n_tiles == 1 && uint32_t(len) <= clg::kZTinySpan) ? 1u : 0u;
  p.spans.push_back(sd);
  p.n_tiles = uint32_t(p.tiles.size());
}

// clg_decode_logs' ranges and device-planned fast plan (plan_log_span's spans, runs and
// segment table, in the same order) on the host threads: per part of the logs their ranges
// and sizes, then the parts' offsets, then each part writes its entries in place.  false:
// not applicable (no device planning) or a log failed -- the caller runs the serial loop,
// which reports the error.
// stage >= 0: the runs, segment table and spans go straight into that decode slot's pinned
// plan buffer (DecodePlan::staged; the spans into p.spans too, which the host reads), so the
// launch copies nothing on the host but the chunk table.
bool clg_engine::plan_parallel(DecodePlan& p, const uint32_t* log, const int64_t* start_epoch, uint32_t n, uint64_t* total,
                               int stage) {
  const uint32_t U = tile_unit(clg::kZTile), Cb = C();
  if (!U) return false;
  WorkPool* wp = workers();
  const unsigned P = wp->size();
  struct Part {
    uint64_t bytes = 0, tiles = 0, runs = 0, segs = 0, tiny = 0;
    bool bad = false;
  };
  std::vector<Part> part(P);
  std::optional<HostTimer> hsub(std::in_place, this, "host_plan_pass1");
  std::vector<int32_t>& st = zst;
  std::vector<int32_t>& nb = znb;
  const uint32_t per = (n + P - 1) / P;
  auto cnt_of = [&](int32_t start, int32_t len) -> uint32_t {
    return len > 0 ? uint32_t(start + len - 1) / U - uint32_t(start) / U + 1 : 0u;
  };
  wp->run([&](unsigned k, unsigned) {
    Part& q = part[k];
    for (uint32_t i = k * per; i < std::min(n, (k + 1) * per); ++i) {
      Log* l;
      if (get_log(log[i], &l) != CLG_OK ||
          (l->depth != 0 && determinants_range(*l, start_epoch[i], &st[i], &nb[i]) != CLG_OK)) {
        q.bad = true;
        return;
      }
      const uint32_t c = cnt_of(st[i], nb[i]);
      q.bytes += uint64_t(nb[i]);
      q.tiles += c;
      q.tiny += (c == 1 && uint32_t(nb[i]) <= clg::kZTinySpan) ? 1u : 0u;
      if (c) {
        ++q.runs;
        q.segs += uint32_t(st[i] + nb[i] - 1) / Cb - uint32_t(st[i]) / Cb + 1;
      }
    }
  });
  std::vector<Part> at(P + 1);
  for (unsigned k = 0; k < P; ++k) {
    if (part[k].bad) return false;
    at[k + 1].bytes = at[k].bytes + part[k].bytes;
    at[k + 1].tiles = at[k].tiles + part[k].tiles;
    at[k + 1].runs = at[k].runs + part[k].runs;
    at[k + 1].segs = at[k].segs + part[k].segs;
    at[k + 1].tiny = at[k].tiny + part[k].tiny;
  }
  if (at[P].tiles >= (1ull << 32)) return false;
  hsub.emplace(this, "host_plan_pass2");
  p.reset();
  p.unit = U;
  p.spans.resize(n);
  p.n_tiles = uint32_t(at[P].tiles);
  p.n_tiny = uint32_t(at[P].tiny);
  clg::SegSpan* runs_out;
  uint32_t* seg_out;
  clg::SpanDesc* spans_copy = nullptr;
  if (stage >= 0) {  // the layout stage_plan computes, room for the count pass's chunk table after it
    PlanLayout L;
    plan_layout(0, at[P].runs * sizeof(clg::SegSpan), at[P].segs * sizeof(uint32_t), size_t(n) * sizeof(clg::SpanDesc),
                (size_t(p.n_tiles) + 2) * sizeof(uint32_t), &L);
    PinBuf& h = h_plan_s[stage];
    if (h.ensure(L.hb + 64) != CLG_OK) return false;
    uint8_t* hd = h.as<uint8_t>();
    runs_out = reinterpret_cast<clg::SegSpan*>(hd + L.o_runs);
    seg_out = reinterpret_cast<uint32_t*>(hd + L.o_seg);
    spans_copy = reinterpret_cast<clg::SpanDesc*>(hd + L.o_spans);
    p.staged = true;
    p.stage_slot = uint32_t(stage);
    p.n_runs = at[P].runs;
    p.n_segs = at[P].segs;
  } else {
    p.runs.resize(at[P].runs);
    p.segtab.resize(at[P].segs);
    runs_out = p.runs.data();
    seg_out = p.segtab.data();
  }
  wp->run([&](unsigned k, unsigned) {
    uint64_t tile = at[k].tiles, run = at[k].runs, seg = at[k].segs;
    for (uint32_t i = k * per; i < std::min(n, (k + 1) * per); ++i) {
      const Log& l = logs[log[i]];
      const int32_t start = st[i], len = nb[i];
      const uint32_t c = cnt_of(start, len);
      p.spans[i] = clg::SpanDesc{uint32_t(tile), c, uint64_t(len)};
      if (spans_copy) spans_copy[i] = p.spans[i];
      if (c) {  // plan_log_span's device-planning entries
        const uint32_t s0 = uint32_t(start) / Cb, s1 = uint32_t(start + len - 1) / Cb + 1;
        runs_out[run++] = clg::SegSpan{seg, uint32_t(start) - s0 * Cb, uint32_t(len), i, uint32_t(tile), 0};
        std::copy(l.segs.begin() + s0, l.segs.begin() + s1, seg_out + seg);
        seg += s1 - s0;
      }
      tile += c;
    }
  });
  *total = at[P].bytes;
  return true;
}

void clg_engine::reset_result(clg_decoded* out) {
  out->n_rec = out->n_wide = 0;
  out->err_status = CLG_OK;
  out->err_span = 0;
  out->err_off = -1;
  out->err_tag = 0;
}

// Uploads the plan's descriptors (spans into d_spans) and materialises its tiles in
// `dtiles` (device planning from the segment table, or the host-built list).
int clg_engine::upload_plan(DecodePlan& p, DevBuf& dtiles) {
  PlanLayout L;
  CHK(stage_plan(p, dtiles, &L));
  return enqueue_plan(p, L, dtiles);
}

// Host half: the plan's descriptors (and the count pass's chunk table, if any) into the
// pinned plan buffer (its own: an asynchronous decode may still be uploading it while later
// calls -- flush, slices -- stage theirs).
void clg_engine::plan_layout(size_t tb, size_t rb, size_t gb, size_t sb, size_t cb, PlanLayout* L) {
  L->tb = tb;
  L->sb = sb;
  L->o_runs = (tb + 15) & ~size_t(15);
  L->o_seg = (L->o_runs + rb + 15) & ~size_t(15);
  L->o_spans = (L->o_seg + gb + 15) & ~size_t(15);
  L->o_chunk = (L->o_spans + sb + 15) & ~size_t(15);
  L->hb = L->o_chunk + cb;
}

int clg_engine::stage_plan(const DecodePlan& p, DevBuf& dtiles, PlanLayout* L, const std::vector<uint32_t>* chunk) {
  const uint32_t nt = p.n_tiles, ns = uint32_t(p.spans.size());
  CHK(dtiles.ensure(std::max<size_t>(1, nt) * sizeof(clg::TileDesc)));
  CHK(d_spans.ensure(ns * sizeof(clg::SpanDesc)));
  const size_t cb = chunk ? chunk->size() * sizeof(uint32_t) : 0;
  plan_layout(p.tiles.size() * sizeof(clg::TileDesc), p.run_count() * sizeof(clg::SegSpan),
              p.seg_count() * sizeof(uint32_t), ns * sizeof(clg::SpanDesc), cb, L);
  PinBuf& h_plan = h_plan_s[plan_slot];
  if (p.staged) {  // runs, segment table and spans are in place (plan_parallel): the chunk table
    if (p.stage_slot != plan_slot || h_plan.cap < L->hb + 64)
      return fail(CLG_E_STATE, "staged decode plan in slot %u, launched in slot %u", p.stage_slot, plan_slot);
    CHK(d_plan.ensure(L->hb));
    if (cb) memcpy(h_plan.as<uint8_t>() + L->o_chunk, chunk->data(), cb);
    return CLG_OK;
  }
  const size_t tb = L->tb, rb = p.runs.size() * sizeof(clg::SegSpan), gb = p.segtab.size() * sizeof(uint32_t),
               sb = L->sb;
  CHK(h_plan.ensure(L->hb + 64));
  CHK(d_plan.ensure(L->hb));
  uint8_t* hd = h_plan.as<uint8_t>();
  if (L->hb >= kParallelCopy) {  // a config-4 plan is ~3 MB: the host threads copy it
    const std::pair<const void*, size_t> part[5] = {
        {p.tiles.data(), tb}, {p.runs.data(), rb}, {p.segtab.data(), gb}, {p.spans.data(), sb},
        {cb ? chunk->data() : nullptr, cb}};
    const size_t dst[5] = {0, L->o_runs, L->o_seg, L->o_spans, L->o_chunk};
    workers()->run([&](unsigned k, unsigned P) {
      for (int j = 0; j < 5; ++j) {
        const size_t n = part[j].second, a = n * k / P, b = n * (k + 1) / P;
        if (b > a) memcpy(hd + dst[j] + a, static_cast<const uint8_t*>(part[j].first) + a, b - a);
      }
    });
    return CLG_OK;
  }
  memcpy(hd, p.tiles.data(), tb);
  memcpy(hd + L->o_runs, p.runs.data(), rb);
  memcpy(hd + L->o_seg, p.segtab.data(), gb);
  memcpy(hd + L->o_spans, p.spans.data(), sb);
  if (cb) memcpy(hd + L->o_chunk, chunk->data(), cb);
  return CLG_OK;
}

// The count pass's chunks of about equal cost: a tile costs its bytes plus a fixed 1 KiB
// (tiles of one span are taken as equally long; a small whole span that pass 0 counted, a
// skip), and block b takes the tiles whose cumulative cost passes b / G of the total.
// ch[0 .. G]: boundaries, ch[G] = n_tiles.
// Batches of many spans: the cost sums per part of the spans on the host threads, then
// each part places the boundaries that fall in it (the same boundaries as one pass).
void clg_engine::count_chunks(const DecodePlan& p, uint32_t G, bool tiny, std::vector<uint32_t>& ch) {
  ch.assign(size_t(G) + 1, p.n_tiles);
  ch[0] = 0;
  constexpr double kTileCost = 1024.0, kTinyCost = 64.0;  // (pass 0 counted the small whole spans)
  auto cost = [&](const clg::SpanDesc& s) {
    return tiny && s.n_tiles == 1 && s.len <= clg::kZTinySpan ? kTinyCost : double(s.len) / s.n_tiles + kTileCost;
  };
  const size_t ns = p.spans.size();
  const unsigned P = ns >= kParallelLogs ? workers()->size() : 1u;
  std::vector<double> part(P + 1, 0.0);
  auto range = [&](unsigned k, size_t* a, size_t* b) {
    *a = ns * k / P;
    *b = ns * (k + 1) / P;
  };
  auto sums = [&](unsigned k, unsigned) {
    size_t a, b;
    range(k, &a, &b);
    double t = 0;
    for (size_t i = a; i < b; ++i)
      if (p.spans[i].n_tiles) t += cost(p.spans[i]) * p.spans[i].n_tiles;
    part[k + 1] = t;
  };
  if (P > 1) workers()->run(sums); else sums(0, 1);
  for (unsigned k = 0; k < P; ++k) part[k + 1] += part[k];
  if (!(part[P] > 0)) return;  // (no tiles)
  const double target = part[P] / G;
  // part k places boundaries [bstart(k), bstart(k + 1)): those past the cost before it
  auto bstart = [&](unsigned k) -> uint32_t {
    if (k == 0) return 1u;
    if (k >= P) return G;
    uint32_t b = uint32_t(std::min<double>(double(G), std::max(1.0, std::floor(part[k] / target))));
    while (b > 1 && target * (b - 1) > part[k]) --b;
    while (b < G && target * b <= part[k]) ++b;
    return b;
  };
  auto place = [&](unsigned k, unsigned) {
    size_t a, e;
    range(k, &a, &e);
    double acc = part[k];
    uint32_t b = bstart(k);
    const uint32_t bend = bstart(k + 1);
    double next = target * b;
    for (size_t i = a; i < e && b < bend; ++i) {
      const auto& s = p.spans[i];
      if (!s.n_tiles) continue;
      const double c = cost(s), end = acc + c * s.n_tiles;
      while (b < bend && next <= end) {  // boundary inside this span: the first tile past it
        const double kk = (next - acc) / c;
        ch[b++] = s.first_tile + std::min<uint32_t>(s.n_tiles, uint32_t(kk) + (kk > double(uint32_t(kk)) ? 1u : 0u));
        next = target * b;
      }
      acc = end;
    }
    const uint32_t past = e < ns ? p.spans[e].first_tile : p.n_tiles;  // (rounding: the part's end)
    while (b < bend) ch[b++] = past;
  };
  if (P > 1) workers()->run(place); else place(0, 1);
}

// Device half: upload, span table, tiles (expanded on the device from the runs).
int clg_engine::enqueue_plan(const DecodePlan& p, const PlanLayout& L, DevBuf& dtiles) {
  HIPCHK(hipMemcpyAsync(d_plan.p, h_plan_s[plan_slot].p, L.hb, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_spans.p, d_plan.as<uint8_t>() + L.o_spans, L.sb, hipMemcpyDeviceToDevice, stream));
  if (!p.runs.empty()) {
    CHK(clg::launch_expand_tiles(reinterpret_cast<const clg::SegSpan*>(d_plan.as<uint8_t>() + L.o_runs),
                                 uint32_t(p.runs.size()), p.n_tiles,
                                 reinterpret_cast<const uint32_t*>(d_plan.as<uint8_t>() + L.o_seg), pool, C(),
                                 p.unit, dtiles.as<clg::TileDesc>(), stream));
  } else if (L.tb) {
    HIPCHK(hipMemcpyAsync(dtiles.p, d_plan.p, L.tb, hipMemcpyDeviceToDevice, stream));
  }
  return CLG_OK;
}

bool clg_engine::mapped_direct(const clg_decoded& out) {
  return out.out_kind == CLG_MEM_MAPPED && out.cap * 13 + out.wcap * 25 <= kMappedDirect &&
         mapped_outputs(out, nullptr);
}

int clg_engine::scratch_out(size_t cap, size_t wcap, clg::DecodeOut* o) {
  CHK(d_o_off.ensure(cap * 4));
  CHK(d_o_tag.ensure(cap));
  CHK(d_o_v0.ensure(cap * 8));
  CHK(d_o_widx.ensure(wcap * 4));
  CHK(d_o_wrc.ensure(wcap * 4));
  CHK(d_o_wv1.ensure(wcap * 8));
  CHK(d_o_wvo.ensure(wcap * 4));
  CHK(d_o_wvl.ensure(wcap * 4));
  CHK(d_o_wsub.ensure(wcap));
  *o = clg::DecodeOut{d_o_off.as<uint32_t>(), d_o_tag.as<uint8_t>(), d_o_v0.as<int64_t>(), d_o_widx.as<uint32_t>(),
                     d_o_wrc.as<int32_t>(), d_o_wv1.as<int64_t>(), d_o_wvo.as<uint32_t>(), d_o_wvl.as<uint32_t>(),
                     d_o_wsub.as<uint8_t>(), 0, 0};
  return CLG_OK;
}

int clg_engine::prep_out(clg_decoded* out, clg::DecodeOut* o) {
  const bool dev = out->out_kind == CLG_MEM_DEVICE;
  if (mapped_direct(*out)) {
    mapped_outputs(*out, o);
    return CLG_OK;
  }
  if (dev) {
    *o = clg::DecodeOut{out->off, out->tag, out->v0, out->w_idx, out->w_rc, out->w_v1, out->w_var_off,
                       out->w_var_len, out->w_sub, out->cap, out->wcap};
  } else {
    CHK(scratch_out(std::max<uint64_t>(1, out->cap), std::max<uint64_t>(1, out->wcap), o));
    o->cap = out->cap, o->wcap = out->wcap;
  }
  return CLG_OK;
}

int clg_engine::finish_out(clg_decoded* out, uint64_t nrec, uint64_t nwide) {
  out->n_rec = nrec;
  out->n_wide = nwide;
  if (out->out_kind != CLG_MEM_DEVICE && !mapped_direct(*out)) {
    // the used part of each array into one pinned staging buffer (asynchronous copies; into
    // the caller's pageable arrays each copy was a synchronous staged transfer: 0.17 ms for
    // config 1's 44-log decode), then into the caller's arrays
    const uint64_t r = std::min(nrec, out->cap), w = std::min(nwide, out->wcap);
    struct Part {
      void* dst;
      const void* src;
      uint64_t n;
    } parts[9] = {{out->off, d_o_off.p, r * 4},          {out->tag, d_o_tag.p, r},
                  {out->v0, d_o_v0.p, r * 8},            {out->w_idx, d_o_widx.p, w * 4},
                  {out->w_rc, d_o_wrc.p, w * 4},         {out->w_v1, d_o_wv1.p, w * 8},
                  {out->w_var_off, d_o_wvo.p, w * 4},    {out->w_var_len, d_o_wvl.p, w * 4},
                  {out->w_sub, d_o_wsub.p, w}};
    uint64_t at[10] = {0};
    for (int i = 0; i < 9; ++i) at[i + 1] = (at[i] + parts[i].n + 15) & ~uint64_t(15);
    if (at[9] <= (uint64_t(64) << 20)) {
      CHK(h_outs.ensure(at[9] + 16));
      uint8_t* hb = h_outs.as<uint8_t>();
      for (int i = 0; i < 9; ++i)
        if (parts[i].n) HIPCHK(hipMemcpyAsync(hb + at[i], parts[i].src, parts[i].n, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      for (int i = 0; i < 9; ++i)
        if (parts[i].n) memcpy(parts[i].dst, hb + at[i], parts[i].n);
    } else {  // large outputs: straight into the caller's arrays (no 64 MB+ pinned buffer)
      for (int i = 0; i < 9; ++i)
        if (parts[i].n) HIPCHK(hipMemcpyAsync(parts[i].dst, parts[i].src, parts[i].n, hipMemcpyDeviceToHost, stream));
    }
  }
  if (settling && out->out_kind == CLG_MEM_DEVICE) {
    collect_timings(true);  // (finish_fused waited for the run's read-back, which follows emit)
  } else {
    CHK(sync());
  }
  if (nrec > out->cap || nwide > out->wcap)
    return fail(CLG_E_CAPACITY, "decode produced %llu records / %llu wide rows, capacity %llu / %llu",
                (unsigned long long)nrec, (unsigned long long)nwide, (unsigned long long)out->cap,
                (unsigned long long)out->wcap);
  return CLG_OK;
}

// Speculative warm-up bytes before each lane's region (CLONOS_WARM overrides; tuning aid).
// Measured on MI355X (tools/r3_warm.sh): 96 B is best for short fixed-length records
// (config 2: count 0.176 ms at 96 B, 0.194 at 64, 0.182 at 128; round 6, with the lean walk
// and the staggered starts, 64-128 B within 2 %: pipeline 0.430-0.437 ms).  With Serializable
// tables the count pass walks the step-code map, whose steps no longer diverge on wide
// records, and 48-128 B are best too (config-3 subset: 0.43-0.44 ms, 0.451 at 16 B).
uint32_t clg_engine::spec_warm() const { return sw.warm >= 0 ? uint32_t(sw.warm) : 96u; }

// Fast three-pass decode (decode_fused.hip).  *aborted = true when the kernels met
// anything outside its fast path; the caller then runs the robust pipeline.
// jser: build the Serializable tables first (phase 3).  *need_jser: the batch aborted
// only because it met Serializable records without tables.
int clg_engine::run_fused(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base, bool* aborted,
                          bool jser, bool* need_jser) {
  *aborted = false;
  *need_jser = false;
  reset_result(out);
  if (p.spans.empty()) return CLG_OK;
  if (!fused_fits(p)) {
    *aborted = true;
    return CLG_OK;
  }
  FusedRun r;
  CHK(launch_fused(p, log_bytes, out, jser, &r));
  return finish_fused(p, r, out, span_rec_base, aborted, need_jser);
}

// Records and wide rows per span from the read-back span_hi words (hz[ns + s], packed
// wide << 31 | records): spans hold consecutive record ranges in span order, so a span's
// range starts where the previous span with tiles ended.  span_rec_base[0 .. ns].
void clg_engine::span_totals(const DecodePlan& p, const uint64_t* hz, uint64_t* span_rec_base, uint64_t* nrec,
                             uint64_t* nwide) {
  constexpr uint64_t kRecMask = (1ull << 31) - 1;
  const uint32_t ns = uint32_t(p.spans.size());
  uint64_t prev = 0;
  for (uint32_t s = 0; s < ns; ++s) {
    if (span_rec_base) span_rec_base[s] = prev & kRecMask;
    if (p.spans[s].n_tiles) prev = hz[ns + s];
  }
  if (span_rec_base) span_rec_base[ns] = prev & kRecMask;
  *nrec = prev & kRecMask;
  *nwide = prev >> 31;
}

// more than 8 GiB in one batch: the offsets pass covers 2^20 tiles
bool clg_engine::fused_fits(const DecodePlan& p) { return p.n_tiles <= (1u << 20); }

int clg_engine::launch_fused(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, bool jser, FusedRun* r) {
  HostTimer ht(this, "host_decode_launch");
  const uint32_t nt = p.n_tiles, ns = uint32_t(p.spans.size());
  r->log_bytes = log_bytes;
  r->jser = jser;
  // chunks of equal cost when blocks take several tiles of spans of different sizes
  const bool zdbg = sw.fused_debug, zprof = !sw.scan_phases.empty();  // developer diagnostics
  // pass 0 (small whole spans, a lane each) for batches without Serializable tables
  const bool tiny = p.n_tiny && !jser && !zprof;
  const uint32_t G = clg::decode_count_grid(jser, nt);
  const bool chunked = G && nt > G && ns > 1;
  std::optional<HostTimer> hsub(std::in_place, this, "host_launch_chunks");  // (CLONOS_HOST_PROF sub-stages)
  if (chunked) count_chunks(p, G, tiny, chunk_buf);
  PlanLayout L;
  hsub.emplace(this, "host_launch_stage");
  struct SlotScope {  // stage_plan / enqueue_plan use this run's slot
    uint32_t& s;
    SlotScope(uint32_t& s_, uint32_t v) : s(s_) { s = v; }
    ~SlotScope() { s = 0; }
  } slot_scope(plan_slot, r->slot);
  CHK(stage_plan(p, d_ztiles, &L, chunked ? &chunk_buf : nullptr));
  hsub.emplace(this, "host_launch_enqueue");
  clg::DecodeOut o{};
  CHK(prep_out(out, &o));
  hsub->lap("host_enq_out");
  // the control words and their read-back: clg::fused_layout, clg::fused_readback (kernels.h)
  const clg::FusedLayout Z = clg::fused_layout(nt, ns, G);
  const clg::FusedReadback RB = clg::fused_readback(ns);
  CHK(d_zctl.ensure(Z.words * 8));
  CHK(d_zbits.ensure(std::max<size_t>(1, nt) * 64 * 16));
  CHK(d_zbad.ensure(std::max<size_t>(1, ns) * 4));
  CHK(d_zerr.ensure(std::max<size_t>(1, ns) * 8));
  PinBuf& h_zres = h_zres_s[r->slot];
  CHK(h_zres.ensure(RB.words * 8));
  hsub->lap("host_enq_bufs");
  uint64_t* w = d_zctl.as<uint64_t>();
  if (zdbg) CHK(d_dbg.ensure(clg::kZDbgTiles * 4 + size_t(nt) * 16));
  if (zprof) CHK(d_prof.ensure(size_t(nt) * 64));
  const uint32_t jwork_cap = std::max<uint32_t>(uint32_t(nt) * 16 + 1024, zjwork_min);
  if (jser) {
    CHK(d_zjpos.ensure((size_t(nt) * clg::kZJCap + zjovf_cap) * 4));
    CHK(d_zjlen.ensure((size_t(nt) * clg::kZJCap + zjovf_cap) * 4));
    CHK(d_zjn.ensure(size_t(nt) * 8));  // jn, jbase
    // (the header, the items' slots and tiles, the sidecar's scan list: its count and tiles)
    CHK(d_zjwork.ensure((clg::kZJWorkHead + 2 * size_t(jwork_cap) + 1 + size_t(nt)) * 4));
  }
  // the scan writes the result into the pinned read-back buffer itself (no copy queued after
  // emit) while the spans are few: each span_hi is its own write across the bus, and for
  // config 4's 66 k spans those took 2.5 ms -- there one copy after emit reads them back
  const bool host_res = ns <= kHostResSpans;
  clg::FusedCtl ctl{};  // (every field, in the struct's order)
  ctl.st_x = w;
  ctl.cnt = w + Z.cnt;
  ctl.base = w + Z.base;
  ctl.boff = w + Z.boff;
  ctl.bits = d_zbits.as<uint64_t>();
  ctl.span_lo = w + Z.span_lo;
  ctl.span_hi = w + Z.span_hi;
  ctl.abort = reinterpret_cast<uint32_t*>(w + Z.abort);
  ctl.dbg = zdbg ? d_dbg.as<uint32_t>() : nullptr;
  ctl.prof = zprof ? d_prof.as<uint64_t>() : nullptr;
  ctl.n_tiles = nt;
  ctl.jpos = jser ? d_zjpos.as<uint32_t>() : nullptr;
  ctl.jlen = jser ? d_zjlen.as<uint32_t>() : nullptr;
  ctl.jn = jser ? d_zjn.as<uint32_t>() : nullptr;
  ctl.jser = jser ? 1u : 0u;
  ctl.jwork_cap = jwork_cap;
  ctl.jwork = jser ? d_zjwork.as<uint32_t>() : nullptr;
  ctl.warm = spec_warm();
  if (jser) CHK(jarena_reset(&ctl.jar));
  ctl.span_bad = d_zbad.as<uint32_t>();
  ctl.skip_bad = 0;
  ctl.chunk = chunked ? reinterpret_cast<const uint32_t*>(d_plan.as<uint8_t>() + L.o_chunk) : nullptr;
  ctl.tiny = tiny ? 1u : 0u;
  ctl.ex = w + Z.ex;
  ctl.rep_flag = reinterpret_cast<uint8_t*>(w + Z.rep_flag);
  ctl.rep = ctl.abort + clg::kZAbortFlagWords;
  ctl.ent = w + Z.ent;
  ctl.perturb = sw.fused_perturb;
  ctl.lb_check = 1;
  ctl.n_spans = ns;
  ctl.span_err = sw.keep_errors ? d_zerr.as<uint64_t>() : nullptr;
  ctl.jbase = jser ? d_zjn.as<uint32_t>() + nt : nullptr;
  ctl.jovf_cap = zjovf_cap;
  ctl.lb = w + Z.lb;
  ctl.h_res = host_res ? h_zres.as<uint64_t>() : nullptr;
  ctl.lean = !jser && (sw.lean >= 0 ? sw.lean != 0 : lean_hint) ? 1u : 0u;
  ctl.side = side;
  memset(h_zres.p, 0, RB.words * 8);  // (a batch without tiles runs no scan)
  hsub->lap("host_enq_memset");
  r->ctl = ctl;
  r->o = o;
  auto* zt = d_ztiles.as<clg::TileDesc>();
  auto* zs = d_spans.as<clg::SpanDesc>();
  const bool timing = (cfg.flags & CLG_F_TIMING) != 0;
  // The whole sequence, enqueued on `stream`; `ev` (timing) brackets jser, count, offsets
  // and emit, `evp` the whole pipeline.  (Captured as a hipGraph and replayed per batch
  // shape it was no faster: 197 us for a 16-log decode either way, and the bench step
  // unchanged.  Split into parts whose count ran beside the previous part's emit on a second
  // stream it was slower: config 2 0.44 -> 0.46 / 0.53 ms in 2 / 4 parts.)
  auto enqueue = [&](hipEvent_t* ev, hipEvent_t* evp) -> int {
    // the plan up in one copy, then one launch for the set-up: tiles from the runs, the span
    // table, and the zeroed control words (st_x, ex, rep_flag; abort words and repair
    // counters; bad-span flags; kept-error offsets ~0; the jser work counters)
    HIPCHK(hipMemcpyAsync(d_plan.p, h_plan_s[plan_slot].p, L.hb, hipMemcpyHostToDevice, stream));
    hsub->lap("host_enq_h2d");
    {
      clg::PrepArgs pa{};
      const bool runs = p.run_count() != 0;
      pa.runs = reinterpret_cast<const clg::SegSpan*>(d_plan.as<uint8_t>() + L.o_runs);
      pa.n_runs = uint32_t(p.run_count());
      pa.n_tiles = runs ? nt : 0;
      pa.segtab = reinterpret_cast<const uint32_t*>(d_plan.as<uint8_t>() + L.o_seg);
      pa.pool = pool;
      pa.C = C();
      pa.U = p.unit;
      pa.tiles = d_ztiles.as<clg::TileDesc>();
      const size_t nsw = std::max<size_t>(1, ns);
      pa.r[0] = clg::PrepRange{d_spans.as<uint32_t>(), reinterpret_cast<const uint32_t*>(d_plan.as<uint8_t>() + L.o_spans),
                               L.sb / 4, 0, 0};
      // (st_x, ex, rep_flag; abort words, repair counters, look-back, entries: fused_layout's two zeroed runs)
      pa.r[1] = clg::PrepRange{reinterpret_cast<uint32_t*>(w), nullptr, 2 * Z.cnt, 0, 0};
      pa.r[2] = clg::PrepRange{ctl.abort, nullptr, 2 * (Z.words - Z.abort), 0, 0};
      pa.r[3] = clg::PrepRange{d_zbad.as<uint32_t>(), nullptr, nsw, 0, 0};
      pa.r[4] = clg::PrepRange{d_zerr.as<uint32_t>(), nullptr, sw.keep_errors ? nsw * 2 : 0, 0xFFFFFFFFu, 0};
      pa.r[5] = clg::PrepRange{ctl.jwork, nullptr, jser ? clg::kZJWorkHead : 0u, 0, 0};
      pa.r[6] = clg::PrepRange{d_ztiles.as<uint32_t>(), reinterpret_cast<const uint32_t*>(d_plan.p), runs ? 0 : L.tb / 4, 0, 0};
      pa.r[7] = clg::PrepRange{jser ? ctl.jwork + clg::kZJWorkHead + 2 * size_t(jwork_cap) : nullptr, nullptr,
                               jser && side.hdr ? 1u : 0u, 0, 0};  // the sidecar's scan-list count
      CHK(clg::launch_decode_prep(pa, stream));
    }
    hsub->lap("host_enq_prep");
    if (zdbg) HIPCHK(hipMemsetAsync(d_dbg.p, 0, clg::kZDbgTiles * 4 + size_t(nt) * 16, stream));
    if (zprof) HIPCHK(hipMemsetAsync(d_prof.p, 0, size_t(nt) * 64, stream));
    if (evp) HIPCHK(hipEventRecord(evp[0], stream));
    if (tiny) CHK(clg::launch_decode_fused(zt, nt, zs, ns, ctl, o, stream, clg::FusedPhase::CountTiny));
    // the passes in launch order, each bracketed by the event pair ev[2 * slot], ev[2 * slot + 1]
    static constexpr struct {
      clg::FusedPhase phase;
      int slot;
    } kPasses[] = {{clg::FusedPhase::JserTables, 0}, {clg::FusedPhase::Count, 1}, {clg::FusedPhase::Scan, 2},
                   {clg::FusedPhase::Emit, 3}};
    for (const auto& ps : kPasses) {
      if (ps.phase == clg::FusedPhase::JserTables && !jser) continue;
      if (ev) HIPCHK(hipEventRecord(ev[2 * ps.slot], stream));
      CHK(clg::launch_decode_fused(zt, nt, zs, ns, ctl, o, stream, ps.phase));
      if (ev) HIPCHK(hipEventRecord(ev[2 * ps.slot + 1], stream));
    }
    if (evp) HIPCHK(hipEventRecord(evp[1], stream));
    hsub->lap("host_enq_kernels");
    // the span ranges and abort words: in h_zres already (the scan wrote them) or read back
    // now (emit ran right behind the scan: it returns at once when the batch aborted, and its
    // stores are bounded by the output capacity)
    if (!host_res) {  // span_hi, the abort words and counters (the host derives the ranges from span_hi)
      HIPCHK(hipMemcpyAsync(h_zres.as<uint64_t>() + RB.span_hi, ctl.span_hi, (RB.jwork - RB.span_hi) * 8,
                            hipMemcpyDeviceToHost, stream));
      if (jser)  // the table work counters beside them (the scan copies them when it writes h_res)
        HIPCHK(hipMemcpyAsync(h_zres.as<uint64_t>() + RB.jwork, ctl.jwork, clg::kZJWorkHead * 4, hipMemcpyDeviceToHost,
                              stream));
    }
    hsub->lap("host_enq_d2h");
    if (jser) CHK(jarena_note(r->note()));
    if (r->slot) {
      if (!zdone[r->slot]) HIPCHK(hipEventCreateWithFlags(&zdone[r->slot], hipEventDisableTiming));
      HIPCHK(hipEventRecord(zdone[r->slot], stream));
      r->done = zdone[r->slot];
    }
    return CLG_OK;
  };
  hipEvent_t ev[8] = {}, evp[2] = {};
  if (timing) {
    for (auto& e : ev) e = get_event();
    for (auto& e : evp) e = get_event();
  }
  CHK(enqueue(timing ? ev : nullptr, timing ? evp : nullptr));
  if (timing) {  // per-kernel durations, read back by sync(); emit's bytes need the record count
    if (jser) timings.push_back(PendingTiming{"decode_jser", ev[0], ev[1], log_bytes});
    else ev_pool.insert(ev_pool.end(), {ev[0], ev[1]});
    timings.push_back(PendingTiming{"decode_count", ev[2], ev[3], log_bytes});
    timings.push_back(PendingTiming{"decode_offsets", ev[4], ev[5], 24 * uint64_t(nt)});
    r->ea = ev[6];
    r->eb = ev[7];
  }
  if (timing) {
    r->pa = evp[0];
    r->pb = evp[1];
  }
  return CLG_OK;
}

// Developer diagnostics: n bytes of device memory at `src`, as they are once the stream's
// queued work is done, into the file `path`.
void clg_engine::dump_device(const std::string& path, const void* src, size_t n) {
  std::vector<uint8_t> h(n);
  if (hipStreamSynchronize(stream) != hipSuccess || hipMemcpy(h.data(), src, n, hipMemcpyDeviceToHost) != hipSuccess)
    return;
  if (FILE* fp = fopen(path.c_str(), "wb")) {
    fwrite(h.data(), 1, n, fp);
    fclose(fp);
  }
}

// CLONOS_FUSED_DEBUG: the diagnostics block of a finished run (clg::ZDbg), printed.  Every
// run: the count pass's chunk-entry reads not taken.  An aborted one: the first tile per
// reason, the first aborting tile's state, a repair walk that gave up.
void clg_engine::print_fused_debug(const DecodePlan& p, const FusedRun& r, const uint32_t* hab, bool aborted) {
  std::vector<uint32_t> hd(clg::kZDbgTiles);
  hipMemcpy(hd.data(), d_dbg.p, hd.size() * 4, hipMemcpyDeviceToHost);
  if (hd[clg::kZDbgSkipN])
    fprintf(stderr, "[clonos] %u chunk-entry reads not taken; first: tile %u word %08x%08x tile span offset %u (poll %u)\n",
            hd[clg::kZDbgSkipN], hd[clg::kZDbgSkipTile], hd[clg::kZDbgSkipWordHi], hd[clg::kZDbgSkipWordLo],
            hd[clg::kZDbgSkipOff], hd[clg::kZDbgSkipPolls]);
  if (!aborted) return;
  fprintf(stderr, "[clonos] fused decode aborted (%u tiles, jser %d): first tile per reason bad=%d end=%d exit=%d "
          "timeout=%d serializable=%d overflow=%d\n", p.n_tiles, int(r.jser), int(~hab[clg::kZAbortBad]),
          int(~hab[clg::kZAbortEnd]), int(~hab[clg::kZAbortExit]), int(~hab[clg::kZAbortTimeout]),
          int(~hab[clg::kZAbortSerializable]), int(~hab[clg::kZAbortOverflow]));
  fprintf(stderr, "[clonos] tile %u reason %u x_pub %u x_true %u e_true %u lo %u hi %u end_a %u\n", hd[clg::kZDbgTile],
          hd[clg::kZDbgReason], hd[clg::kZDbgMustExit], hd[clg::kZDbgXTrue], hd[clg::kZDbgETrue], hd[clg::kZDbgLo],
          hd[clg::kZDbgHi], hd[clg::kZDbgEndA]);
  if (hd[clg::kZDbgWalkMark] == clg::kZDbgWalkGaveUp) {
    const uint32_t f = hd[clg::kZDbgWalkFrom], at = hd[clg::kZDbgWalkAt];
    fprintf(stderr, "[clonos] repair walk from tile %u gave up at tile %u (entry %u exit %u, span %u, %u disagreements)\n",
            f, at, hd[clg::kZDbgWalkEntry], hd[clg::kZDbgWalkExit], hd[clg::kZDbgWalkSpan], hd[clg::kZDbgWalkDisagree]);
    // who wrote the exits before the walk (site 1 the count pass, 2 a repair walk)
    std::vector<uint64_t> pp(size_t(p.n_tiles) * 2);
    hipMemcpy(pp.data(), d_dbg.as<uint32_t>() + clg::kZDbgTiles, pp.size() * 8, hipMemcpyDeviceToHost);
    for (uint32_t t = f >= 10 ? f - 10 : 0; t <= std::min(at + 1, p.n_tiles - 1); ++t) {
      const uint64_t w = pp[size_t(t) * 2 + 1];
      uint64_t exv = 0, stx = 0;
      hipMemcpy(&exv, r.ctl.ex + t, 8, hipMemcpyDeviceToHost);
      hipMemcpy(&stx, r.ctl.st_x + t, 8, hipMemcpyDeviceToHost);
      fprintf(stderr, "[clonos]   tile %u: ex writer site %llu block %llu (chunk first / walk start %llu, why/old %llu) "
              "entry %llu ex %llx st_x %llx\n",
              t, (unsigned long long)(w >> 60), (unsigned long long)((w >> 32) & 0xFFFFFFF),
              (unsigned long long)((w >> 4) & 0xFFFFFF), (unsigned long long)(w & 15),
              (unsigned long long)pp[size_t(t) * 2], (unsigned long long)exv, (unsigned long long)stx);
    }
  }
  for (int l = 0; l < 64; ++l) {
    const uint32_t* d = &hd[clg::kZDbgLanes + clg::kZDbgLaneWords * l];
    fprintf(stderr, "  lane %2d rs %5u re %5u spec_exit %5u spec_bad %5u canon_exit %5u canon_bad %u entry %5u exit %5u bad %u\n",
            l, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7] & 0x7FFFFFFFu, d[7] >> 31);
  }
}

// A queued run's result: wait, counters, grown tables, abort classification, totals.
int clg_engine::finish_fused(const DecodePlan& p, FusedRun& r, clg_decoded* out, uint64_t* span_rec_base, bool* aborted,
                             bool* need_jser) {
  *aborted = false;
  *need_jser = false;
  const uint32_t nt = p.n_tiles, ns = uint32_t(p.spans.size());
  const bool jser = r.jser;
  const uint64_t log_bytes = r.log_bytes;
  hipEvent_t ea = r.ea, eb = r.eb;
  uint64_t* hz = h_zres_s[r.slot].as<uint64_t>();
  {
    HostTimer hw(this, "host_decode_wait");
    if (r.done) HIPCHK(hipEventSynchronize(r.done));  // (a later decode may be queued behind it)
    else HIPCHK(hipStreamSynchronize(stream));
  }
  HostTimer ht(this, "host_decode_finish");
  if (!sw.scan_phases.empty()) dump_device(sw.scan_phases, d_prof.p, size_t(nt) * 64);
  const uint32_t* hab = reinterpret_cast<const uint32_t*>(hz + clg::fused_readback(ns).abort);
  auto rep = [&](clg::ZRep k) { return hab[clg::zhab_rep(k)]; };
  if (jser) jser_hint = hab[clg::kZAbortJserSeen] != 0;  // keep building tables while batches hold Serializable records
  // repair requests the count pass served, chunks walked again for a wrong entry, canonical
  // exits inside their tile
  if (const uint32_t n = rep(clg::kZRepFiled)) stats["decode_chunk_repair"].launches += n;
  if (const uint32_t n = rep(clg::kZRepServed)) stats["decode_entry_repair"].launches += n;
  if (const uint32_t n = rep(clg::kZRepCanonEarly)) stats["decode_canon_before_end"].launches += n;
  const bool spilled = jser && jarena_spilled(r.note());  // a stream walk found the spill arena full
  if (spilled) CHK(jarena_grow());
  // Serializable tables: the overflow arena or the walker's work list was full
  bool grown = false;
  if (jser && hab[clg::kZAbortOverflow]) {
    // the work list's and the overflow arena's use, from this run's own read-back (a later
    // decode queued behind it may have zeroed the device words already)
    const uint32_t items = hab[clg::kZHabJWork + clg::kZJWorkItems], ovf = hab[clg::kZHabJWork + clg::kZJWorkOvf];
    if (items > r.ctl.jwork_cap) zjwork_min = std::max(zjwork_min, 2 * items);
    if (ovf > zjovf_cap) zjovf_cap = std::max<uint32_t>(2 * ovf, 2 * zjovf_cap);
    grown = items > r.ctl.jwork_cap || ovf > r.ctl.jovf_cap;
    stats["decode_jser_grow"].launches++;
  }
  const bool gave_up = hab[clg::kZAbortAny] || spilled;
  if (sw.fused_debug) print_fused_debug(p, r, hab, gave_up);
  if (gave_up) {
    if (ea) {
      ev_pool.push_back(ea);
      ev_pool.push_back(eb);
    }
    if (r.pa) {
      ev_pool.push_back(r.pa);
      ev_pool.push_back(r.pb);
    }
    *aborted = true;
    for (uint32_t k = 0; k < clg::kZAbortFlagWords; ++k)  // (which reasons: the bench line lists them beside the kernels)
      if (clg::kZAbortStat[k] && hab[k]) stats[clg::kZAbortStat[k]].launches++;
    // Serializable records were met without tables: other aborts may be consequences
    // (entries guessed across them), so the tables decide; a second abort goes robust
    // (a table arena that was full, now grown: the same, once)
    *need_jser = (!jser && hab[clg::kZAbortSerializable] && !spilled) || (jser && (spilled || grown));
    r.lookback_bad = rep(clg::kZRepLookback) != 0;  // a look-back read gave a wrong offset
    r.span_local =
        !*need_jser && !spilled && !hab[clg::kZAbortTimeout] && !hab[clg::kZAbortOverflow] && !r.lookback_bad;
    if (r.lookback_bad) stats["decode_lookback_check"].launches++;
    zlast = r;
    return CLG_OK;
  }
  uint64_t nrec = 0, nwide = 0;
  span_totals(p, hz, span_rec_base, &nrec, &nwide);
  if (!jser) lean_hint = nwide * 16 < nrec;
  if (ea) timings.push_back(PendingTiming{"decode_emit", ea, eb, log_bytes + 13 * nrec + 25 * nwide});
  // the pipeline's algorithmic bytes: log bytes read + the SoA rows
  if (r.pa) timings.push_back(PendingTiming{"decode_pipeline", r.pa, r.pb, log_bytes + 13 * nrec + 25 * nwide});
  return finish_out(out, nrec, nwide);
}

bool clg_engine::small_ok(const DecodePlan& p, uint64_t log_bytes, const clg_decoded* out) const {
  if (!small_decode || jser_hint || p.spans.empty() || p.spans.size() > kSmallSpans || log_bytes > kSmallBytes ||
      p.only || p.staged)
    return false;
  if (out->out_kind == CLG_MEM_HOST && out->cap * 13 + out->wcap * 25 > kSmallHostOut) return false;
  if (out->out_kind == CLG_MEM_MAPPED && !mapped_outputs(*out, nullptr)) return false;
  return p.n_tiles <= clg::kZSmallTilesMax;
}

// CLG_MEM_MAPPED outputs: every array's device address (false: one is not registered, or
// its cap / wcap elements reach past its registered range -- the caller's staging path then)
bool clg_engine::mapped_outputs(const clg_decoded& out, clg::DecodeOut* o) {
  void* h[9] = {out.off, out.tag, out.v0, out.w_idx, out.w_rc, out.w_v1, out.w_var_off, out.w_var_len, out.w_sub};
  const uint64_t c = std::max<uint64_t>(1, out.cap), w = std::max<uint64_t>(1, out.wcap);
  const uint64_t n[9] = {c * 4, c, c * 8, w * 4, w * 4, w * 8, w * 4, w * 4, w};
  uintptr_t d[9];
  for (int i = 0; i < 9; ++i)
    if (!(d[i] = clg_mapped_device_address(h[i], n[i]))) return false;
  if (o)
    *o = clg::DecodeOut{reinterpret_cast<uint32_t*>(d[0]), reinterpret_cast<uint8_t*>(d[1]), reinterpret_cast<int64_t*>(d[2]),
                        reinterpret_cast<uint32_t*>(d[3]), reinterpret_cast<int32_t*>(d[4]), reinterpret_cast<int64_t*>(d[5]),
                        reinterpret_cast<uint32_t*>(d[6]), reinterpret_cast<uint32_t*>(d[7]), reinterpret_cast<uint8_t*>(d[8]),
                        out.cap, out.wcap};
  return true;
}

// The plan's device-planned runs as host-built tiles (k_expand_tiles' rule, on the host).
void clg_engine::host_tiles(DecodePlan& p) {
  if (p.runs.empty()) return;
  const uint32_t U = p.unit, Cb = C();
  p.tiles.resize(p.n_tiles);
  for (const auto& r : p.runs) {
    const uint32_t w0 = r.phys / U, w1 = (r.phys + r.len - 1) / U;
    for (uint32_t w = w0; w <= w1; ++w) {
      const uint32_t s0 = std::max(w * U, r.phys), e1 = std::min((w + 1) * U, r.phys + r.len);
      const uint32_t si = s0 / Cb, so = s0 % Cb;
      p.tiles[r.first + (w - w0)] = clg::TileDesc{seg_addr(segtab_at(p, r.segtab_off + si)) + (so & ~15u), so & 15u,
                                                  e1 - s0, uint32_t(r.dst), 0, uint64_t(s0 - r.phys)};
    }
  }
  p.runs.clear();
  p.segtab.clear();
  p.unit = 0;
}

uint32_t clg_engine::segtab_at(const DecodePlan& p, uint64_t i) { return p.segtab[size_t(i)]; }

// The small path's hand-offs, checked once its kernel is done: every tile but a span's first
// entered at the exit the tile before it published, and every tile's base is the one before
// it plus that tile's counts (the kernel's per-tile words: entry | exit << 32, base, counts).
// A mismatch -- a poll that read a wrong word -- sends the batch the usual way.
bool clg_engine::small_handoffs_ok(const DecodePlan& p, const uint64_t* res) {
  const uint32_t nt = p.n_tiles, ns = uint32_t(p.spans.size());
  for (uint32_t t = 0; t < nt; ++t) {
    const uint64_t* k = res + clg::small_check_at(ns, t);
    const uint64_t* q = k - clg::kZSmallCheckWords;  // the tile before's (t > 0)
    const bool first = p.tiles[t].span_off == 0;
    const uint64_t base = t == 0 ? 0 : q[clg::kZCheckBase] + q[clg::kZCheckCount];
    if (k[clg::kZCheckBase] != base ||
        (!first && uint32_t(k[clg::kZCheckEntryExit]) != uint32_t(q[clg::kZCheckEntryExit] >> 32))) {
      stats["decode_small_handoff"].launches++;
      return false;
    }
  }
  return true;
}

int clg_engine::run_small(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base, bool* aborted) {
  HostTimer ht(this, "host_decode_small");
  *aborted = false;
  reset_result(out);
  host_tiles(p);
  const uint32_t nt = p.n_tiles, ns = uint32_t(p.spans.size());
  if (nt == 0) {  // every span empty: no records, and no launch (a grid of zero blocks is invalid)
    if (span_rec_base) std::fill(span_rec_base, span_rec_base + ns + 1, uint64_t(0));
    out->n_rec = out->n_wide = 0;
    return CLG_OK;
  }
  // the plan: in the launch's arguments when it fits (no copy queued), else one copy
  const bool arg_plan = nt <= clg::kZSmallArgTiles && ns <= clg::kZSmallArgSpans;
  PlanLayout L;
  if (arg_plan) {
    memcpy(small_arg.tiles, p.tiles.data(), size_t(nt) * sizeof(clg::TileDesc));
    memcpy(small_arg.spans, p.spans.data(), size_t(ns) * sizeof(clg::SpanDesc));
  } else {
    CHK(stage_plan(p, d_ztiles, &L));
  }
  // outputs: the caller's device arrays, or pinned host memory the kernel writes directly
  clg::DecodeOut o{};
  const bool host = out->out_kind == CLG_MEM_HOST;
  const uint64_t cap = std::max<uint64_t>(1, out->cap), wcap = std::max<uint64_t>(1, out->wcap);
  uint64_t at[10] = {0};
  const uint64_t sz[9] = {cap * 4, cap, cap * 8, wcap * 4, wcap * 4, wcap * 8, wcap * 4, wcap * 4, wcap};
  for (int i = 0; i < 9; ++i) at[i + 1] = (at[i] + sz[i] + 15) & ~uint64_t(15);
  if (host) {
    CHK(h_small_out.ensure(at[9] + 16));
    uint8_t* hb = h_small_out.as<uint8_t>();
    o = clg::DecodeOut{reinterpret_cast<uint32_t*>(hb + at[0]), hb + at[1], reinterpret_cast<int64_t*>(hb + at[2]),
                       reinterpret_cast<uint32_t*>(hb + at[3]), reinterpret_cast<int32_t*>(hb + at[4]),
                       reinterpret_cast<int64_t*>(hb + at[5]), reinterpret_cast<uint32_t*>(hb + at[6]),
                       reinterpret_cast<uint32_t*>(hb + at[7]), hb + at[8], out->cap, out->wcap};
  } else if (out->out_kind == CLG_MEM_MAPPED) {  // registered host memory: written from the GPU directly
    mapped_outputs(*out, &o);
  } else {
    o = clg::DecodeOut{out->off, out->tag, out->v0, out->w_idx, out->w_rc, out->w_v1, out->w_var_off,
                       out->w_var_len, out->w_sub, out->cap, out->wcap};
  }
  // scratch: per-tile counts and record-start bitmaps, per-span look-back words
  CHK(d_zbits.ensure(std::max<size_t>(1, nt) * 64 * 16));
  CHK(h_small_res.ensure(clg::small_res_words(ns, nt) * 8));
  uint64_t* res = h_small_res.as<uint64_t>();
  res[clg::kZSmallRec] = res[clg::kZSmallWide] = res[clg::kZSmallFailed] = 0;
  // look-back words: two buffers of kZSmallAggWords, zeroed once; each call zeroes the other;
  // then the per-tile counts
  constexpr size_t kAgg = clg::kZSmallAggWords;
  if (!d_small.p) {
    CHK(d_small.ensure((2 * kAgg + clg::kZSmallTilesMax) * 8));
    HIPCHK(hipMemsetAsync(d_small.p, 0, 2 * kAgg * 8, stream));
  }
  uint64_t* agg = d_small.as<uint64_t>() + (small_flip ? kAgg : 0);
  uint64_t* agg_next = d_small.as<uint64_t>() + (small_flip ? 0 : kAgg);
  small_flip = !small_flip;
  uint64_t* cnt = d_small.as<uint64_t>() + 2 * kAgg;
  clg::FusedCtl ctl{};
  ctl.cnt = cnt;
  ctl.bits = d_zbits.as<uint64_t>();
  ctl.n_tiles = nt;
  ctl.n_spans = ns;
  ctl.perturb = sw.fused_perturb;
  // warm-up 32 B, not staggered: a lone wave per span waits on every step, and shorter
  // warm-ups cost fewer merges than they save (config 1: the kernel 65 -> 62 us at 32 or 16 B,
  // 63 at 48)
  ctl.warm = 32u | (1u << 31);
  const bool sprof = sw.small_prof;  // developer diagnostics: phase stamps
  if (sprof) {
    CHK(d_prof.ensure(size_t(nt) * 64));
    HIPCHK(hipMemsetAsync(d_prof.p, 0, size_t(nt) * 64, stream));
    ctl.prof = d_prof.as<uint64_t>();
  }
  std::optional<HostTimer> hsub(std::in_place, this, "host_small_submit");  // (CLONOS_HOST_PROF sub-stages)
  if (!arg_plan) HIPCHK(hipMemcpyAsync(d_plan.p, h_plan_s[0].p, L.hb, hipMemcpyHostToDevice, stream));
  const bool timing = (cfg.flags & CLG_F_TIMING) != 0;
  hipEvent_t ea = nullptr, eb = nullptr;
  if (timing) {
    ea = get_event();
    eb = get_event();
    HIPCHK(hipEventRecord(ea, stream));
  }
  CHK(clg::launch_decode_small(reinterpret_cast<const clg::TileDesc*>(d_plan.p), nt,
                               reinterpret_cast<const clg::SpanDesc*>(d_plan.as<uint8_t>() + L.o_spans), ns, ctl, o,
                               agg, agg_next, res, stream, arg_plan ? &small_arg : nullptr));
  if (timing) HIPCHK(hipEventRecord(eb, stream));
  hsub.emplace(this, "host_small_wait");
  HIPCHK(hipStreamSynchronize(stream));
  hsub.emplace(this, "host_small_finish");
  if (sprof) {  // per tile (count_tile's stamps): walk, merge, counts ticks; merge steps, passes
    std::vector<uint64_t> hp(size_t(nt) * 8);
    HIPCHK(hipMemcpy(hp.data(), d_prof.p, hp.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t t = 0; t < nt; ++t) {
      const uint64_t* q = &hp[size_t(t) * 8];
      fprintf(stderr, "[clonos] small decode tile %u: walk %llu  merge %llu  counts %llu  steps %llu/%llu  passes %llu\n", t,
              (unsigned long long)(q[2] - q[1]), (unsigned long long)(q[3] - q[2]), (unsigned long long)(q[4] - q[3]),
              (unsigned long long)(q[5] & 0xFFFFF), (unsigned long long)((q[5] >> 20) & 0xFFFFF),
              (unsigned long long)(q[5] >> 40));
    }
  }
  if (res[clg::kZSmallFailed] || !small_handoffs_ok(p, res)) {
    if (timing) timings.push_back(PendingTiming{"decode_small", ea, eb, 0});
    *aborted = true;
    return CLG_OK;
  }
  constexpr uint64_t kRecMask = (1ull << 31) - 1;
  const uint64_t nrec = res[clg::kZSmallRec], nwide = res[clg::kZSmallWide];
  if (span_rec_base) {
    for (uint32_t s = 0; s < ns; ++s) span_rec_base[s] = res[clg::kZSmallSpan0 + s] & kRecMask;
    span_rec_base[ns] = nrec;
    for (uint32_t s = ns; s-- > 0;)  // (the kernel writes the spans with tiles: an empty one starts where the next does)
      if (!p.spans[s].n_tiles) span_rec_base[s] = span_rec_base[s + 1];
  }
  if (timing) timings.push_back(PendingTiming{"decode_small", ea, eb, log_bytes + 13 * nrec + 25 * nwide});
  out->n_rec = nrec;
  out->n_wide = nwide;
  if (host) {
    const uint64_t r = std::min(nrec, out->cap), w = std::min(nwide, out->wcap);
    const uint8_t* hb = h_small_out.as<uint8_t>();
    void* dst[9] = {out->off, out->tag, out->v0, out->w_idx, out->w_rc, out->w_v1, out->w_var_off, out->w_var_len,
                    out->w_sub};
    const uint64_t n[9] = {r * 4, r, r * 8, w * 4, w * 4, w * 8, w * 4, w * 4, w};
    for (int i = 0; i < 9; ++i)
      if (n[i]) memcpy(dst[i], hb + at[i], n[i]);
  }
  if (nrec > out->cap || nwide > out->wcap)
    return fail(CLG_E_CAPACITY, "decode produced %llu records / %llu wide rows, capacity %llu / %llu",
                (unsigned long long)nrec, (unsigned long long)nwide, (unsigned long long)out->cap,
                (unsigned long long)out->wcap);
  return CLG_OK;
}

// Decode dispatcher: fused single pass first, robust pipeline on abort.  `build(plan,
// tile_bytes)` fills a plan for the given tile geometry.
int clg_engine::decode(const PlanBuild& build, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base,
                       DecodePlan* prebuilt) {
  // fused counts are packed in 31-bit fields: at most log_bytes / 2 records
  if (fused_decode && log_bytes / 2 < (1ull << 31)) {
    DecodePlan own;
    DecodePlan& pf = prebuilt ? *prebuilt : own;  // (prebuilt: the fast plan, kZTile tiles)
    if (!prebuilt) {
      HostTimer hp(this, "host_decode_plan");
      build(pf, clg::kZTile);
    }
    CHK(plan_ok(pf));
    bool aborted = false, need_jser = false;
    if (small_ok(pf, log_bytes, out)) {
      CHK(run_small(pf, log_bytes, out, span_rec_base, &aborted));
      if (!aborted) return CLG_OK;
      stats["decode_small_fallback"].launches++;
    }
    CHK(run_fused(pf, log_bytes, out, span_rec_base, &aborted, jser_hint, &need_jser));
    if (!aborted) return CLG_OK;
    return after_abort(pf, build, log_bytes, out, span_rec_base, need_jser);
  }
  DecodePlan p;
  build(p, uint32_t(clg::kTile));
  CHK(plan_ok(p));
  return run_decode(p, log_bytes, out, span_rec_base);
}

int clg_engine::plan_ok(const DecodePlan& p) {
  return p.status == CLG_OK ? CLG_OK
                            : fail(p.status, "a queued decode's log range is gone (truncated past its start epoch)");
}

int clg_engine::span_fallback(DecodePlan& pf, const PlanBuild& build, uint64_t log_bytes, clg_decoded* out,
                              uint64_t* span_rec_base, bool* done) {
  *done = false;
  const uint32_t ns = uint32_t(pf.spans.size()), nt = pf.n_tiles;
  std::vector<uint32_t> flag(ns);
  HIPCHK(hipMemcpy(flag.data(), d_zbad.p, size_t(ns) * 4, hipMemcpyDeviceToHost));
  // spans with an error position (kept errors): the full rules classify the record there on
  // the GPU; a confirmed error keeps the fast run's records before it (k_err_classify)
  std::vector<uint32_t> kept;
  std::vector<uint64_t> kept_off;
  std::vector<int32_t> kept_res;
  if (zlast.ctl.span_err) {
    std::vector<uint64_t> err(ns);
    HIPCHK(hipMemcpy(err.data(), zlast.ctl.span_err, size_t(ns) * 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> cand;
    for (uint32_t s = 0; s < ns; ++s)
      if (flag[s] && err[s] != ~0ull) cand.push_back(s);
    if (!cand.empty()) {
      const uint32_t nc = uint32_t(cand.size());
      CHK(d_sf_cls.ensure(size_t(nc) * 12 + 64));
      HIPCHK(hipMemcpyAsync(d_sf_cls.p, cand.data(), size_t(nc) * 4, hipMemcpyHostToDevice, stream));
      auto* cres = reinterpret_cast<int32_t*>(d_sf_cls.as<uint8_t>() + ((size_t(nc) * 4 + 15) & ~size_t(15)));
      clg::JArena jar;
      CHK(jarena_reset(&jar));
      CHK(clg::launch_err_classify(d_ztiles.as<clg::TileDesc>(), d_spans.as<clg::SpanDesc>(), d_sf_cls.as<uint32_t>(),
                                   nc, zlast.ctl, cres, jar, stream));
      std::vector<int32_t> cr(size_t(nc) * 2);
      HIPCHK(hipMemcpyAsync(cr.data(), cres, cr.size() * 4, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      for (uint32_t i = 0; i < nc; ++i)
        if (cr[2 * i] < 0) {  // confirmed: not a bad span any more
          flag[cand[i]] = 0;
          kept.push_back(cand[i]);
          kept_off.push_back(err[cand[i]]);
          kept_res.push_back(cr[2 * i]);
          kept_res.push_back(cr[2 * i + 1]);
        }
    }
  }
  std::vector<uint32_t> bad;
  uint64_t bad_bytes = 0;
  for (uint32_t s = 0; s < ns; ++s)
    if (flag[s]) {
      bad.push_back(s);
      bad_bytes += pf.spans[s].len;
    }
  if ((bad.empty() && kept.empty()) || bad.size() > kSfMaxSpans || bad_bytes > log_bytes / 4 * 3) return CLG_OK;
  if (!kept.empty()) stats["decode_kept_errors"].launches++;
  if (!bad.empty()) stats["decode_span_fallback"].launches++;
  const uint32_t nb = uint32_t(bad.size());
  // scratch: the robust decode's records (13 B) and wide rows (25 B) of the bad spans
  const uint64_t RC = bad_bytes / 2 + nb + 1, WC = bad_bytes / 6 + nb + 1;  // (records are >= 2 B, wide >= 6 B)
  CHK(d_sf_rec.ensure(RC * 13 + 64));
  CHK(d_sf_wide.ensure(WC * 25 + 64));
  uint8_t* rb = d_sf_rec.as<uint8_t>();
  uint8_t* wb = d_sf_wide.as<uint8_t>();
  auto* s_off = reinterpret_cast<uint32_t*>(rb);
  auto* s_v0 = reinterpret_cast<int64_t*>(rb + RC * 4 + 7 - (RC * 4 + 7) % 8);
  auto* s_tag = reinterpret_cast<uint8_t*>(s_v0 + RC);
  auto* s_widx = reinterpret_cast<uint32_t*>(wb);
  auto* s_wrc = reinterpret_cast<int32_t*>(s_widx + WC);
  auto* s_wvo = reinterpret_cast<uint32_t*>(s_wrc + WC);
  auto* s_wvl = s_wvo + WC;
  auto* s_wv1 = reinterpret_cast<int64_t*>(reinterpret_cast<uint8_t*>(s_wvl + WC) + 8 - (uintptr_t(s_wvl + WC) & 7));
  auto* s_wsub = reinterpret_cast<uint8_t*>(s_wv1 + WC);
  std::vector<uint64_t> packed(nb), nrec(nb), nwide(nb), rbase(nb), wbase(nb);
  int e_status = CLG_OK, e_tag = 0;
  uint32_t e_span = 0;
  int64_t e_off = -1;
  if (nb) {  // every bad span in ONE robust run (spans 0 .. nb-1 of its plan), into scratch
    DecodePlan sp;
    sp.only = &bad;
    build(sp, uint32_t(clg::kTile));
    CHK(plan_ok(sp));
    clg_decoded so{};
    so.off = s_off;
    so.tag = s_tag;
    so.v0 = s_v0;
    so.w_idx = s_widx;
    so.w_rc = s_wrc;
    so.w_v1 = s_wv1;
    so.w_var_off = s_wvo;
    so.w_var_len = s_wvl;
    so.w_sub = s_wsub;
    so.cap = RC;
    so.wcap = WC;
    so.out_kind = CLG_MEM_DEVICE;
    const int st = run_decode(sp, bad_bytes, &so, nullptr);
    if (st != CLG_OK && so.err_status == CLG_OK) return st;  // an engine failure, not a decode error
    if (so.err_status != CLG_OK) {  // the lowest bad span's error (bad[] ascends)
      e_status = so.err_status;
      e_span = bad[so.err_span];
      e_off = so.err_off;
      e_tag = so.err_tag;
    }
    // per span: records, wide rows and their places in the scratch (run_decode's span results)
    const clg::SpanRes* hres = h_sres.as<clg::SpanRes>();
    for (uint32_t i = 0; i < nb; ++i) {
      nrec[i] = hres[i].n_rec;
      nwide[i] = hres[i].n_wide;
      rbase[i] = hres[i].rec_base;
      wbase[i] = hres[i].wide_base;
      if (nrec[i] >= (1ull << 31) || nwide[i] >= (1ull << 32)) return CLG_OK;  // past the fast counts' packing
      packed[i] = nwide[i] << 31 | nrec[i];
    }
  }
  // the lowest span's error: the robust run's or a kept one's (kept[] ascends)
  if (!kept.empty() && (e_status == CLG_OK || kept[0] < e_span)) {
    e_status = kept_res[0];
    e_span = kept[0];
    e_off = int64_t(kept_off[0]);
    e_tag = kept_res[1];
  }
  // the fast run again over the good spans: its plan back in place (the robust runs used
  // the shared span table), the bad spans' counts injected, scan and emit (kept errors: the
  // tiles past the error hold no records, emit stops there)
  PlanLayout L;
  if (nb) {
    CHK(stage_plan(pf, d_ztiles, &L));
    CHK(enqueue_plan(pf, L, d_ztiles));
  }
  // meta: the packed counts, the bad spans, then the placement rows (16-byte aligned)
  const size_t o_place = (size_t(nb) * 12 + 15) & ~size_t(15), mb = o_place + size_t(nb) * sizeof(clg::SfPlace);
  CHK(d_sf_meta.ensure(mb + 64));
  std::vector<uint8_t> meta(mb + 8);
  memcpy(meta.data(), packed.data(), size_t(nb) * 8);
  memcpy(meta.data() + size_t(nb) * 8, bad.data(), size_t(nb) * 4);
  auto* pl = reinterpret_cast<clg::SfPlace*>(meta.data() + o_place);
  for (uint32_t i = 0; i < nb; ++i) pl[i] = clg::SfPlace{rbase[i], nrec[i], wbase[i], nwide[i], bad[i], 0};
  HIPCHK(hipMemcpyAsync(d_sf_meta.p, meta.data(), mb, hipMemcpyHostToDevice, stream));
  clg::FusedCtl ctl = zlast.ctl;
  ctl.skip_bad = 1;
  ctl.lb_check = 0;  // (the three-launch scan below: no look-back words)
  ctl.chunk = nullptr;  // (the count pass's chunk table is not staged again: scan and emit never read it)
  auto* zt = d_ztiles.as<clg::TileDesc>();
  auto* zs = d_spans.as<clg::SpanDesc>();
  CHK(clg::launch_decode_inject(zs, reinterpret_cast<const uint32_t*>(d_sf_meta.as<uint8_t>() + size_t(nb) * 8),
                                d_sf_meta.as<uint64_t>(), nb, ctl, stream));
  HIPCHK(hipMemsetAsync(ctl.abort, 0, clg::kZAbortFlagWords * 4, stream));
  CHK(clg::launch_decode_fused(zt, nt, zs, ns, ctl, zlast.o, stream, clg::FusedPhase::Scan3));
  CHK(clg::launch_decode_fused(zt, nt, zs, ns, ctl, zlast.o, stream, clg::FusedPhase::Emit));
  // the robust records into place, at the bases the scan gave the bad spans (one launch)
  const clg::DecodeOut sc{s_off, s_tag, s_v0, s_widx, s_wrc, s_wv1, s_wvo, s_wvl, s_wsub, RC, WC};
  CHK(clg::launch_sf_place(reinterpret_cast<const clg::SfPlace*>(d_sf_meta.as<uint8_t>() + o_place), nb, sc, zlast.o,
                           ctl, stream));
  const clg::FusedReadback RB = clg::fused_readback(ns);
  CHK(h_zres_s[0].ensure(RB.words * 8));
  uint64_t* hz = h_zres_s[0].as<uint64_t>();
  HIPCHK(hipMemcpyAsync(hz, ctl.span_lo, RB.abort_only * 8, hipMemcpyDeviceToHost, stream));  // ranges, abort flag words
  HIPCHK(hipStreamSynchronize(stream));
  if (reinterpret_cast<const uint32_t*>(hz + RB.abort)[clg::kZAbortAny]) return CLG_OK;  // (cannot happen) whole batch
  uint64_t tr = 0, tw = 0;
  span_totals(pf, hz, span_rec_base, &tr, &tw);
  *done = true;
  CHK(finish_out(out, tr, tw));
  if (e_status != CLG_OK) {
    out->err_status = e_status;
    out->err_span = e_span;
    out->err_off = e_off;
    out->err_tag = e_tag;
    return fail(e_status, "decode error %d in span %u at offset %lld (tag %d)", e_status, e_span, (long long)e_off,
                e_tag);
  }
  return CLG_OK;
}

// The fast path aborted: again with the Serializable length tables when that was the
// reason; then, when only some spans' chains went wrong, those spans alone through the
// robust pipeline (span_fallback); else the whole batch through it.
int clg_engine::after_abort(DecodePlan& pf, const PlanBuild& build, uint64_t log_bytes, clg_decoded* out,
                            uint64_t* span_rec_base, bool need_jser) {
  bool aborted = true, nj = false;
  if (pf.staged) {  // its runs and segment table live only in the pinned buffer: planned again
    pf.reset();
    build(pf, clg::kZTile);
    CHK(plan_ok(pf));
  }
  // a look-back read gave a wrong offset (emit's check): the fast path once more, as it was
  if (zlast.lookback_bad && !need_jser) {
    CHK(run_fused(pf, log_bytes, out, span_rec_base, &aborted, zlast.jser, &nj));
    if (!aborted) return CLG_OK;
    need_jser = nj;
  }
  // with the tables; again (at most twice) while a table arena was full and has grown
  for (int tries = 0; need_jser && tries < 3; ++tries) {
    stats["decode_jser_retry"].launches++;
    CHK(run_fused(pf, log_bytes, out, span_rec_base, &aborted, true, &nj));
    if (!aborted) return CLG_OK;
    need_jser = nj;
  }
  if (zlast.span_local && !nj) {
    bool done = false;
    const int st = span_fallback(pf, build, log_bytes, out, span_rec_base, &done);
    if (done) return st;
  }
  stats["decode_fallback"].launches++;
  DecodePlan p;
  build(p, uint32_t(clg::kTile));
  CHK(plan_ok(p));
  return run_decode(p, log_bytes, out, span_rec_base);
}

void clg_engine::release_later() {
  if (free_later.empty() || any_active()) return;
  free_segs.insert(free_segs.end(), free_later.begin(), free_later.end());
  free_later.clear();
}

bool clg_engine::any_active(size_t from) const {
  for (size_t i = from; i < pq.size(); ++i)
    if (pq[i].active) return true;
  return false;
}

// A decode the async call completed at once (not queued): its status goes to the wait.
// Engine failures (not a decode result) return from the call instead, with nothing queued.
int clg_engine::push_settled(int st, clg_decoded* out) {
  if (st != CLG_OK && st != CLG_E_CAPACITY && out->err_status == CLG_OK) return st;
  PendingDecode d;
  d.status = st;
  if (st != CLG_OK) d.err = g_err;
  pq.push_back(std::move(d));
  return CLG_OK;
}

int clg_engine::decode_async(PlanBuild build, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base,
                             DecodePlan* prebuilt) {
  const bool fast = fused_decode && log_bytes / 2 < (1ull << 31);
  DecodePlan pf;
  if (prebuilt) {
    pf = std::move(*prebuilt);  // (the fast plan, kZTile tiles)
  } else if (fast) {
    HostTimer hp(this, "host_decode_plan");
    build(pf, clg::kZTile);
  }
  CHK(plan_ok(pf));
  const bool queue = fast && !pf.spans.empty() && fused_fits(pf);
  // what the queued decodes' completions need must not be overwritten by this one's kernels:
  // host outputs go through shared staging arrays, and a scratch buffer that has to grow
  // frees the old one
  bool clash = !queue;
  for (const auto& d : pq)
    if (d.active && d.out->out_kind != CLG_MEM_DEVICE) clash = true;
  if (queue && (pf.n_tiles > hw_tiles || pf.spans.size() > hw_spans || pf.run_count() > hw_runs ||
                pf.seg_count() > hw_segs || (jser_hint && !hw_jser)))
    clash = true;
  if (clash) CHK(settle());
  if (!queue) {  // nothing to queue, or too large for the fast path: decoded now
    if (fast && pf.spans.empty()) {
      reset_result(out);
      return push_settled(CLG_OK, out);
    }
    return push_settled(decode(build, log_bytes, out, span_rec_base), out);
  }
  reset_result(out);
  // a slot no queued decode holds: the one the plan was staged for (free still: planned in
  // this call, and a settle above only frees slots)
  const uint32_t slot = pf.staged ? pf.stage_slot : free_slot();
  if (slot == 0 || slot >= kSlots || slot_used(slot))
    return fail(CLG_E_STATE, "no free decode slot");  // (cannot happen: bounded by the caller)
  FusedRun r;
  r.slot = slot;
  CHK(launch_fused(pf, log_bytes, out, jser_hint, &r));
  hw_tiles = std::max<uint64_t>(hw_tiles, pf.n_tiles);
  hw_spans = std::max<uint64_t>(hw_spans, pf.spans.size());
  hw_runs = std::max<uint64_t>(hw_runs, pf.run_count());
  hw_segs = std::max<uint64_t>(hw_segs, pf.seg_count());
  hw_jser = hw_jser || r.jser;
  PendingDecode d;
  d.active = true;
  d.plan = std::move(pf);
  d.run = r;
  d.log_bytes = log_bytes;
  d.out = out;
  d.span_rec_base = span_rec_base;
  d.build = std::move(build);
  d.min_epoch = q_min_epoch;
  pq.push_back(std::move(d));
  return CLG_OK;
}

bool clg_engine::slot_used(uint32_t slot) const {
  for (const auto& d : pq)
    if (d.active && d.run.slot == slot) return true;
  return false;
}

uint32_t clg_engine::free_slot() const {  // the first asynchronous decode slot no queued decode holds (kSlots: none)
  uint32_t slot = 1;
  while (slot < kSlots && slot_used(slot)) ++slot;
  return slot;
}

// Completes the queued decodes [0, upto] (all: upto = SIZE_MAX), oldest first.
int clg_engine::settle(size_t upto) {
  for (size_t i = 0; i < pq.size() && i <= upto; ++i) {
    PendingDecode& d = pq[i];
    if (!d.active) continue;
    d.active = false;
    int st;
    if (d.redo) {  // a decode before it aborted after this one was queued
      CHK(sync());
      st = decode(d.build, d.log_bytes, d.out, d.span_rec_base);
    } else {
      bool aborted = false, need_jser = false;
      settling = true;
      st = finish_fused(d.plan, d.run, d.out, d.span_rec_base, &aborted, &need_jser);
      settling = false;
      if (st == CLG_OK && aborted) {
        if (any_active(i + 1)) {  // its scratch went to the later decodes: all of them again
          stats["decode_async_redo"].launches++;
          CHK(sync());
          for (size_t j = i + 1; j < pq.size(); ++j)
            if (pq[j].active) pq[j].redo = true;
          st = decode(d.build, d.log_bytes, d.out, d.span_rec_base);
        } else {
          st = after_abort(d.plan, d.build, d.log_bytes, d.out, d.span_rec_base, need_jser);
        }
      }
    }
    d.status = st;
    if (st != CLG_OK) d.err = g_err;
    d.build = nullptr;
    if (plan_pool.size() < kSlots) {
      d.plan.reset();
      plan_pool.push_back(std::move(d.plan));
    }
    d.plan = DecodePlan();
  }
  release_later();
  return CLG_OK;  // the decodes' own statuses go to clg_decode_wait
}

// clg_decode_wait: the oldest queued decode, completed; its status
int clg_engine::wait_oldest(std::string* err) {
  if (pq.empty()) return CLG_OK;
  CHK(settle(0));
  const int st = pq.front().status;
  if (st != CLG_OK) *err = pq.front().err;
  pq.pop_front();
  release_later();
  return st;
}

// The robust pipeline; again with a grown spill arena while a Serializable stream walk
// found the arena full (CLG_E_NOSPACE is never a decode result).
int clg_engine::run_decode(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base) {
  for (;;) {
    CHK(jarena_clear_note(0));
    const int st = run_decode_once(p, log_bytes, out, span_rec_base);
    if (!jarena_spilled(0)) return st;
    CHK(jarena_grow());
  }
}

int clg_engine::run_decode_once(DecodePlan& p, uint64_t log_bytes, clg_decoded* out, uint64_t* span_rec_base) {
  reset_result(out);
  const uint32_t nt = p.n_tiles, ns = uint32_t(p.spans.size());
  if (ns == 0) return CLG_OK;
  CHK(d_agg.ensure(std::max<size_t>(1, nt) * clg::kEntries * sizeof(uint64_t)));
  CHK(d_conv.ensure(std::max<size_t>(1, nt) * sizeof(clg::TileConv)));
  CHK(d_tres.ensure(std::max<size_t>(1, nt) * sizeof(clg::TileRes)));
  CHK(d_sres.ensure(ns * sizeof(clg::SpanRes)));
  CHK(d_totals.ensure(2 * sizeof(uint64_t)));
  CHK(d_fconv.ensure(std::max<size_t>(1, nt) * clg::kFPoints * sizeof(uint32_t)));
  CHK(d_lanes.ensure(std::max<size_t>(1, nt) * clg::kFPoints * sizeof(clg::LaneSeg)));
  CHK(d_sums.ensure(std::max<size_t>(1, nt) * sizeof(clg::TileSum)));
  CHK(d_fres.ensure(std::max<size_t>(1, nt) * sizeof(clg::FastRes)));
  CHK(d_flags.ensure(ns * sizeof(uint32_t)));
  CHK(d_jpos.ensure(std::max<size_t>(1, nt) * clg::kJserCap * sizeof(uint32_t)));
  CHK(d_jlen.ensure(std::max<size_t>(1, nt) * clg::kJserCap * sizeof(uint32_t)));
  CHK(d_jn.ensure(std::max<size_t>(1, nt) * sizeof(uint32_t)));
  CHK(d_defer.ensure(std::max<size_t>(1, nt) * sizeof(uint32_t)));
  CHK(upload_plan(p, d_tiles));
  CHK(h_sres.ensure(ns * sizeof(clg::SpanRes) + 64));
  clg::DecodeOut o{};
  CHK(prep_out(out, &o));
  auto* dt = d_tiles.as<clg::TileDesc>();
  auto* ds = d_spans.as<clg::SpanDesc>();
  auto* flags = d_flags.as<uint32_t>();
  // fast path: fused scan (points + segments) -> per-span resolution -> emit
  clg::JArena jar;
  CHK(jarena_reset(&jar));
  clg::JserTabs J{d_jpos.as<uint32_t>(), d_jlen.as<uint32_t>(), d_jn.as<uint32_t>(), d_defer.as<uint32_t>(), jar};
  J.side = side;  // (k_jser_fill takes a tile's table from the sidecar where it can)
  const std::string& rprof_path = sw.robust_phases;  // developer diagnostics (stamps per tile)
  if (!rprof_path.empty() && d_rprof.ensure(std::max<size_t>(1, nt) * 16 * 8) == CLG_OK) {
    J.prof = d_rprof.as<uint64_t>();
    hipMemsetAsync(J.prof, 0, size_t(nt) * 128, stream);
  }
  uint32_t* dbg = nullptr;
  if (!sw.debug_dump.empty() && d_dbg.ensure(std::max<size_t>(1, nt) * clg::kFPoints * 4) == CLG_OK)
    dbg = d_dbg.as<uint32_t>();
  uint64_t* prof = nullptr;  // developer diagnostics: per-phase s_memtime stamps of the scan
  if (!sw.scan_phases.empty() && d_prof.ensure(std::max<size_t>(1, nt) * 8 * 8) == CLG_OK) {
    prof = d_prof.as<uint64_t>();
    hipMemsetAsync(prof, 0, size_t(nt) * 64, stream);
  }
  CHK(timed("robust_scan", log_bytes, [&] {
    return clg::launch_fast_scan(dt, nt, ds, d_fconv.as<uint32_t>(), J, 0, d_lanes.as<clg::LaneSeg>(),
                                 d_sums.as<clg::TileSum>(), dbg, prof, stream);
  }));
  if (prof) dump_device(sw.scan_phases, prof, size_t(nt) * 64);
  CHK(timed("robust_jser", 0, [&] { return clg::launch_jser_fill(dt, nt, ds, J, stream); }));
  uint64_t* prof2 = nullptr;  // developer diagnostics: the deferred scan's phase stamps (CLONOS_ROBUST_PHASES)
  if (J.prof && d_prof2.ensure(std::max<size_t>(1, nt) * 64) == CLG_OK) {
    prof2 = d_prof2.as<uint64_t>();
    hipMemsetAsync(prof2, 0, size_t(nt) * 64, stream);
  }
  CHK(timed("robust_scan_deferred", 0, [&] {
    return clg::launch_fast_scan(dt, nt, ds, d_fconv.as<uint32_t>(), J, 1, d_lanes.as<clg::LaneSeg>(),
                                 d_sums.as<clg::TileSum>(), dbg, prof2, stream);
  }));
  if (prof2) dump_device(rprof_path + ".scan", prof2, size_t(nt) * 64);
  CHK(timed("robust_resolve", uint64_t(nt) * 32, [&] {
    return clg::launch_fast_resolve(dt, ds, ns, d_fconv.as<uint32_t>(), d_lanes.as<clg::LaneSeg>(),
                                    d_sums.as<clg::TileSum>(), J, d_fres.as<clg::FastRes>(),
                                    d_sres.as<clg::SpanRes>(), flags, jar, stream);
  }));
  if (cfg.flags & CLG_F_TIMING) {  // diagnostics: spans the convergence-point tier leaves to the DP
    std::vector<uint32_t> hf(ns);
    HIPCHK(hipMemcpyAsync(hf.data(), flags, size_t(ns) * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    uint64_t nf = 0, no = 0;
    for (uint32_t f : hf) {
      nf += f != 0;
      no += f == 2;
    }
    stats["robust_dp_spans"].launches += nf;
    stats["robust_dp_spans_overflow"].launches += no;
    stats["robust_spans"].launches += ns;
  }
  // robust DP pipeline for flagged spans only (early exit elsewhere)
  CHK(timed("robust_dp_tables", 0, [&] {
    return clg::launch_decode_tables(dt, nt, ds, d_agg.as<uint64_t>(), d_conv.as<clg::TileConv>(), flags, jar, stream);
  }));
  CHK(timed("robust_dp_resolve", 0, [&] {
    return clg::launch_decode_resolve(dt, ds, ns, d_agg.as<uint64_t>(), d_conv.as<clg::TileConv>(),
                                      d_tres.as<clg::TileRes>(), d_sres.as<clg::SpanRes>(), flags, jar, stream);
  }));
  CHK(timed("robust_spanscan", uint64_t(ns) * 48, [&] {
    return clg::launch_decode_spanscan(d_sres.as<clg::SpanRes>(), ns, d_totals.as<uint64_t>(), stream);
  }));
  // emit bytes are attributed after the counts are known (below)
  hipEvent_t ea = nullptr, eb = nullptr;
  if (cfg.flags & CLG_F_TIMING) {
    ea = get_event();
    eb = get_event();
    hipEventRecord(ea, stream);
  }
  CHK(clg::launch_fast_emit(dt, nt, ds, d_fconv.as<uint32_t>(), J, d_lanes.as<clg::LaneSeg>(),
                            d_fres.as<clg::FastRes>(), d_sres.as<clg::SpanRes>(), flags, o, stream));
  if (cfg.flags & CLG_F_TIMING) hipEventRecord(eb, stream);
  CHK(timed("robust_dp_emit", 0, [&] {
    return clg::launch_decode_emit(dt, nt, ds, d_conv.as<clg::TileConv>(), d_tres.as<clg::TileRes>(),
                                   d_sres.as<clg::SpanRes>(), flags, o, jar, stream);
  }));
  if (J.prof) dump_device(rprof_path, J.prof, size_t(nt) * 128);
  if (!sw.debug_dump.empty()) {  // developer diagnostics only: the robust scan's state in one file
    hipStreamSynchronize(stream);
    if (FILE* fp = fopen(sw.debug_dump.c_str(), "wb")) {
      std::vector<uint8_t> h;
      auto put = [&](const void* dev, size_t n) {  // n bytes of device memory
        h.resize(n);
        hipMemcpy(h.data(), dev, n, hipMemcpyDeviceToHost);
        fwrite(h.data(), 1, n, fp);
      };
      fwrite(&nt, 4, 1, fp);
      fwrite(&ns, 4, 1, fp);
      put(d_fconv.p, size_t(nt) * clg::kFPoints * 4);
      put(d_sums.p, size_t(nt) * sizeof(clg::TileSum));
      put(d_flags.p, size_t(ns) * 4);
      put(d_tiles.p, size_t(nt) * sizeof(clg::TileDesc));
      put(d_dbg.p, size_t(nt) * clg::kFPoints * 4);
      put(d_lanes.p, size_t(nt) * clg::kFPoints * sizeof(clg::LaneSeg));
      fclose(fp);
    }
  }
  clg::SpanRes* hres = h_sres.as<clg::SpanRes>();
  HIPCHK(hipMemcpyAsync(hres, d_sres.p, ns * sizeof(clg::SpanRes), hipMemcpyDeviceToHost, stream));
  CHK(jarena_note(0));
  HIPCHK(hipStreamSynchronize(stream));
  uint64_t nrec = 0, nwide = 0;
  for (uint32_t s = 0; s < ns; ++s) {
    if (span_rec_base) span_rec_base[s] = hres[s].rec_base;
    nrec += hres[s].n_rec;
    nwide += hres[s].n_wide;
    if (hres[s].status != CLG_OK && out->err_status == CLG_OK) {
      out->err_status = hres[s].status;
      out->err_span = s;
      out->err_off = hres[s].err_off;
      out->err_tag = hres[s].err_tag;
    }
  }
  if (span_rec_base) span_rec_base[ns] = nrec;
  if (cfg.flags & CLG_F_TIMING)
    timings.push_back(PendingTiming{"robust_emit", ea, eb, log_bytes + 13 * nrec + 25 * nwide});
  CHK(finish_out(out, nrec, nwide));
  if (out->err_status != CLG_OK)
    return fail(out->err_status, "decode error %d in span %u at offset %lld (tag %d)", out->err_status, out->err_span,
                (long long)out->err_off, out->err_tag);
  return CLG_OK;
}

extern "C" {

int clg_decode_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len, uint32_t n,
                    clg_decoded* out, uint64_t* span_rec_base) {
  ENGINE_GUARD(e);
  if (!out || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) total += span_len[i];
  const uint8_t* base;  // span i starts at base + (span_off[i] - base_off)
  uint64_t base_off;
  CHK(e->stage_spans(bytes, span_off, span_len, n, CLG_MEM_HOST, &base, &base_off));
  auto build = [&](clg_engine::DecodePlan& p, uint32_t T) {
    for (uint32_t i = 0; i < n; ++i)
      e->plan_host_span(p, base + (span_len[i] ? span_off[i] - base_off : 0), span_len[i], i, T);
  };
  return e->decode(build, total, out, span_rec_base);
}

int clg_decode_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, clg_decoded* out,
                    uint64_t* span_rec_base) {
  ENGINE_GUARD(e);
  if (!out || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  CHK(e->flush());
  std::vector<int32_t>& st = e->zst;
  std::vector<int32_t>& nb = e->znb;
  st.assign(n, 0);
  nb.assign(n, 0);
  uint64_t total = 0;
  // the ranges and the fast decode's plan in one pass over the logs (per-log work of a
  // 66 k-log batch is bound by the cache misses on the log records)
  clg_engine::DecodePlan& pf = e->zplan;
  pf.reset();
  if (e->fused_decode) {
    pf.spans.reserve(n);
    pf.runs.reserve(n);
  }
  {
    clg_engine::HostTimer ht(e, "host_decode_plan");
    if (!(n >= clg_engine::kParallelLogs && e->fused_decode && e->plan_parallel(pf, log, start_epoch, n, &total, 0))) {
      total = 0;
      pf.reset();
      for (uint32_t i = 0; i < n; ++i) {
        Log* l;
        CHK(e->get_log(log[i], &l));
        if (l->depth != 0) CHK(e->determinants_range(*l, start_epoch[i], &st[i], &nb[i]));
        total += uint64_t(nb[i]);
        if (e->fused_decode) e->plan_log_span(pf, *l, st[i], nb[i], i, clg::kZTile);
      }
    }
  }
  auto build = [&](clg_engine::DecodePlan& p, uint32_t T) {  // re-plans (fallbacks)
    p.spans.reserve(n);
    p.runs.reserve(n);
    for (uint32_t i = 0; i < n; ++i) e->plan_log_span(p, e->logs[log[i]], st[i], nb[i], i, T);
  };
  return e->decode(build, total, out, span_rec_base, e->fused_decode ? &pf : nullptr);
}

int clg_decode_logs_async(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                          clg_decoded* out, uint64_t* span_rec_base) {
  ENGINE_GUARD_KEEP(e);  // (the queued decodes stay queued)
  if (!out || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  // every queued decode's status is kept for its wait
  if (e->pq.size() >= CLG_DECODE_MAX_INFLIGHT)
    return fail(CLG_E_STATE, "%d asynchronous decodes are not waited for (clg_decode_wait)", CLG_DECODE_MAX_INFLIGHT);
  CHK(e->flush());  // (stream-ordered after the queued decodes, past their ranges)
  std::vector<uint32_t> hs(log, log + n);
  std::vector<int32_t> st, nb;
  uint64_t total = 0;
  // many logs: the ranges and the fast plan on the host threads (clg_decode_logs' way), into
  // a recycled plan
  clg_engine::DecodePlan pf;
  if (!e->plan_pool.empty()) {
    pf = std::move(e->plan_pool.back());
    e->plan_pool.pop_back();
  }
  pf.reset();
  bool planned = false;
  if (n >= clg_engine::kParallelLogs && e->fused_decode) {
    clg_engine::HostTimer ht(e, "host_decode_plan");
    e->zst.assign(n, 0);  // (plan_parallel's ranges go here)
    e->znb.assign(n, 0);
    const uint32_t fs = e->free_slot();  // (the plan is staged for that slot)
    planned = e->plan_parallel(pf, log, start_epoch, n, &total, fs < clg_engine::kSlots ? int(fs) : -1);
  }
  if (planned) {
    st.assign(e->zst.begin(), e->zst.begin() + n);
    nb.assign(e->znb.begin(), e->znb.begin() + n);
  } else {
    total = 0;
    st.assign(n, 0);
    nb.assign(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
      Log* l;
      CHK(e->get_log(log[i], &l));
      if (l->depth != 0) CHK(e->determinants_range(*l, start_epoch[i], &st[i], &nb[i]));
      total += uint64_t(nb[i]);
    }
  }
  // by value: the robust fallback may re-plan when the decode is settled.  Only a checkpoint
  // truncation at or below every start epoch runs before that (clg_truncate_all settles
  // otherwise); it rebases the logs, and a re-plan after it looks the ranges up again (the
  // same bytes at their new offsets)
  int64_t mn = INT64_MAX;
  for (uint32_t i = 0; i < n; ++i) mn = std::min(mn, start_epoch[i]);
  std::vector<int64_t> eps(start_epoch, start_epoch + n);
  auto build = [e, hs = std::move(hs), st = std::move(st), nb = std::move(nb), eps = std::move(eps),
                gen = e->rebase_gen](clg_engine::DecodePlan& p, uint32_t T) {
    p.spans.reserve(hs.size());
    p.runs.reserve(hs.size());
    for (uint32_t i = 0; i < uint32_t(hs.size()); ++i) {
      int32_t s = st[i], b = nb[i];
      const Log& l = e->logs[hs[i]];
      if (gen != e->rebase_gen && l.depth != 0 && e->determinants_range(l, eps[i], &s, &b) != CLG_OK) {
        p.status = CLG_E_STATE;  // (the settle-on-truncate rule makes this unreachable)
        s = b = 0;
      }
      e->plan_log_span(p, l, s, b, i, T);
    }
  };
  e->q_min_epoch = n ? mn : INT64_MAX;
  const int rc = e->decode_async(build, total, out, span_rec_base, planned ? &pf : nullptr);
  e->q_min_epoch = INT64_MIN;
  if (pf.spans.capacity() && e->plan_pool.size() < clg_engine::kSlots) {  // (not queued: the plan back)
    pf.reset();
    e->plan_pool.push_back(std::move(pf));
  }
  return rc;
}

int clg_decode_wait(clg_engine* e) {
  ENGINE_GUARD_KEEP(e);
  std::string err;
  const int st = e->wait_oldest(&err);
  return st == CLG_OK ? CLG_OK : fail(st, "%s", err.c_str());
}

}  // extern "C"
