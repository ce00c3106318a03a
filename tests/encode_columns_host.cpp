// Stand-alone check of the CPU encode of typed columns (clonos_amd/csrc/encode_columns.h):
// seeded batches built record by record next to their expected bytes (written here field by
// field, not through the header's writers), every span split, sizes only, the capacity failure
// with guard bytes, and each error kind with its lowest index.  Built with g++ (no HIP), plainly
// and with -fsanitize=address,undefined; every array is allocated at its exact size so that a
// read or write past a stated length is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../clonos_amd/csrc/encode_columns.h"

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

struct Batch {
  std::vector<uint8_t> tag, w_sub, var;
  std::vector<int8_t> order;
  std::vector<int64_t> timestamp, w_v1, w_v0;
  std::vector<int32_t> rng, buffer_built, w_rc;
  std::vector<uint32_t> w_var_len, w_idx;
  std::vector<uint64_t> pos, span_base, rec_bytes;  // rec_bytes[i]: the byte offset of record i
  std::vector<uint8_t> want;

  void be(uint64_t v, int w) {
    for (int k = w - 1; k >= 0; --k) want.push_back(uint8_t(v >> (8 * k)));
  }
  void row() {
    span_base.insert(span_base.end(), {order.size(), timestamp.size(), rng.size(), buffer_built.size(), w_v0.size()});
  }
  void add(std::mt19937_64& r) {
    const uint32_t t = uint32_t(r() % 8);
    rec_bytes.push_back(want.size());
    tag.push_back(uint8_t(t));
    want.push_back(uint8_t(t));
    const int64_t v = int64_t(r());
    if (t == 0) { order.push_back(int8_t(v)); be(uint8_t(v), 1); return; }
    if (t == 1) { timestamp.push_back(v); be(uint64_t(v), 8); return; }
    if (t == 2) { rng.push_back(int32_t(v)); be(uint32_t(v), 4); return; }
    if (t == 7) { buffer_built.push_back(int32_t(v)); be(uint32_t(v), 4); return; }
    const int32_t rc = int32_t(r());
    const int64_t v1 = int64_t(r());
    static const uint32_t lens[] = {0, 1, 15, 16, 17, 63, 64, 65, 300};
    uint32_t len = lens[r() % 9];
    uint32_t sub = uint32_t(r() % 7);
    if (t == 5) sub = uint32_t(r() % 4) | (r() % 2 ? 0x80u : 0u);
    w_idx.push_back(uint32_t(tag.size() - 1));
    w_rc.push_back(rc), w_v1.push_back(v1), w_v0.push_back(v), w_sub.push_back(uint8_t(sub)), w_var_len.push_back(len);
    pos.back() = var.size();
    const bool pay = t == 3 || (t == 4 && sub == 6) || (t == 5 && (sub & 0x80));
    if (t != 3) be(uint32_t(rc), 4), be(uint64_t(v), 8);
    if (t == 4) be(sub, 1);
    if (t == 5) be(uint64_t(v1), 8), be(sub & 0x7F, 1), be(sub >> 7, 1);
    if (pay && t != 3) be(len, 4);
    // rows without a payload keep their w_var_len (it must not be read as one) and hold bytes in
    // var all the same, as the decode's rows may
    for (uint32_t k = 0; k < len; ++k) {
      var.push_back(uint8_t(r()));
      if (pay) want.push_back(var.back());
    }
    pos.push_back(var.size());
  }
};

Batch make(uint64_t seed, uint32_t n, const std::vector<uint32_t>& cuts) {  // cuts: record indices where spans start
  std::mt19937_64 r(seed);
  Batch b;
  b.pos.push_back(0);
  size_t c = 0;
  for (uint32_t i = 0; i < n; ++i) {
    while (c < cuts.size() && cuts[c] == i) b.row(), ++c;
    b.add(r);
  }
  b.rec_bytes.push_back(b.want.size());
  while (c < cuts.size()) b.row(), ++c;
  b.row();  // the totals
  return b;
}

// Exact-size copies on the heap: the sanitizer sees a read past any stated length.
template <class T>
T* exact(const std::vector<T>& v) {
  T* p = static_cast<T*>(malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0)));
  for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  return p;
}

struct In {
  clg_columns_in in{};
  std::vector<void*> owned;
  template <class T>
  const T* own(const std::vector<T>& v) {
    T* p = exact(v);
    owned.push_back(p);
    return p;
  }
  In(const Batch& b, bool spans, bool idx) {
    in.tag = own(b.tag), in.order = own(b.order), in.timestamp = own(b.timestamp), in.rng = own(b.rng);
    in.buffer_built = own(b.buffer_built), in.w_rc = own(b.w_rc), in.w_v1 = own(b.w_v1);
    in.w_var_len = own(b.w_var_len), in.w_sub = own(b.w_sub), in.w_v0 = own(b.w_v0);
    in.w_idx = idx ? own(b.w_idx) : nullptr;
    in.pos = own(b.pos), in.var = own(b.var);
    in.n_rec = b.tag.size();
    const uint64_t nc[5] = {b.order.size(), b.timestamp.size(), b.rng.size(), b.buffer_built.size(), b.w_v0.size()};
    for (int c = 0; c < 5; ++c) in.n_class[c] = nc[c];
    in.n_var = b.var.size();
    if (spans) in.span_base = own(b.span_base), in.n_spans = uint32_t(b.span_base.size() / 5 - 1);
    in.in_kind = CLG_MEM_HOST;
  }
  ~In() {
    for (void* p : owned) free(p);
  }
};

void check_ok(const Batch& b, const std::vector<uint32_t>& cuts, bool spans, bool idx) {
  In x(b, spans, idx);
  const uint32_t ns = spans ? uint32_t(cuts.size()) : 1;
  std::vector<uint64_t> sbb(ns + 1, ~0ull);
  clg_encoded out{};
  out.span_byte_base = sbb.data();
  REQUIRE(clg::ecol_build_host(&x.in, &out) == CLG_OK);  // sizes only
  REQUIRE(out.n_bytes == b.want.size() && out.bad_what == CLG_ENC_BAD_NONE && out.bad_index == ~0ull);
  for (uint32_t s = 0; s <= ns; ++s) {
    const uint64_t want = !spans ? (s ? b.want.size() : 0) : s < ns ? b.rec_bytes[cuts[s]] : b.want.size();
    REQUIRE(sbb[s] == want);
  }
  // exact capacity
  uint8_t* buf = static_cast<uint8_t*>(malloc(b.want.size() + 1));
  out.bytes = buf, out.cap = b.want.size();
  REQUIRE(clg::ecol_build_host(&x.in, &out) == CLG_OK);
  for (size_t i = 0; i < b.want.size(); ++i) REQUIRE(buf[i] == b.want[i]);
  // one byte short: the results filled, nothing written
  if (!b.want.empty()) {
    for (size_t i = 0; i < b.want.size(); ++i) buf[i] = 0xA5;
    out.cap = b.want.size() - 1, out.n_bytes = 0;
    REQUIRE(clg::ecol_build_host(&x.in, &out) == CLG_E_CAPACITY);
    REQUIRE(out.n_bytes == b.want.size());
    for (size_t i = 0; i < b.want.size(); ++i) REQUIRE(buf[i] == 0xA5);
  }
  free(buf);
}

int run_bad(In& x, uint32_t* what, uint64_t* index) {
  uint8_t guard[8] = {0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5};
  clg_encoded out{};
  out.bytes = guard, out.cap = 0;  // (nothing may be written)
  const int st = clg::ecol_build_host(&x.in, &out);
  for (uint8_t g : guard) REQUIRE(g == 0xA5);
  *what = out.bad_what, *index = out.bad_index;
  return st;
}

void check_errors(const Batch& b, const std::vector<uint32_t>& cuts) {
  uint32_t what;
  uint64_t index;
  const uint64_t n = b.tag.size(), nw = b.w_v0.size();
  if (n >= 3) {  // two bad tags: the lower one
    Batch c = b;
    c.tag[n - 1] = 9, c.tag[n / 2] = 8;
    In x(c, true, true);
    REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_TAG && index == n / 2);
  }
  for (int cls = 0; cls < 5; ++cls) {  // a stated count one above the tags' (the column itself is not read past its length)
    In x(b, false, false);
    x.in.n_class[cls] += 1;
    if (cls == 4) continue;  // (the wide rows' arrays would have to grow: covered below with one fewer)
    REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_TOTALS && index == uint64_t(cls));
  }
  if (nw) {  // a stated wide count one below: class 4
    In x(b, false, false);
    x.in.n_class[4] -= 1;
    REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_TOTALS && index == 4);
  }
  // rows: two payload rows past n_var (the lower one), and a w_idx that names another record
  std::vector<uint64_t> pay;
  for (uint64_t k = 0; k < nw; ++k) {
    const uint32_t t = b.tag[b.w_idx[k]], sub = b.w_sub[k];
    if ((t == 3 || (t == 4 && sub == 6) || (t == 5 && (sub & 0x80))) && b.w_var_len[k]) pay.push_back(k);
  }
  if (pay.size() >= 2) {
    Batch c = b;
    c.pos[pay.back()] = c.var.size(), c.pos[pay[pay.size() / 2]] = ~0ull - 3;  // (pos + len wraps in 64 bits)
    In x(c, true, true);
    REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_ROW && index == pay[pay.size() / 2]);
  }
  if (nw >= 2) {
    Batch c = b;
    c.w_idx[nw - 1] += 1, c.w_idx[1] += 1;
    In x(c, true, true);
    REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_ROW && index == 1);
    In y(c, true, false);  // not given: not checked
    clg_encoded out{};
    REQUIRE(clg::ecol_build_host(&y.in, &out) == CLG_OK && out.n_bytes == b.want.size());
  }
  // a row without a payload may carry any pos and length
  for (uint64_t k = 0; k < nw; ++k) {
    const uint32_t t = b.tag[b.w_idx[k]], sub = b.w_sub[k];
    if (t == 3 || (t == 4 && sub == 6) || (t == 5 && (sub & 0x80))) continue;
    Batch c = b;
    c.pos[k] = ~0ull, c.w_var_len[k] = ~0u;
    In x(c, true, true);
    clg_encoded out{};
    REQUIRE(clg::ecol_build_host(&x.in, &out) == CLG_OK && out.n_bytes == b.want.size());
    break;
  }
  // spans: a decreasing row, a last row that is not the totals, a row that is not the tags' counts
  const uint32_t ns = uint32_t(cuts.size());
  if (ns >= 3 && n >= 8) {
    {
      Batch c = b;
      for (int k = 0; k < 5; ++k) c.span_base[2 * 5 + k] = 0;  // row 2 below row 1 (when row 1 is not zero)
      bool dec = false;
      for (int k = 0; k < 5; ++k) dec = dec || c.span_base[5 + k] > 0;
      In x(c, true, true);
      if (dec) REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_SPAN && index == 1);
    }
    {
      Batch c = b;
      c.span_base[size_t(ns) * 5] += 1;
      In x(c, true, true);
      REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_SPAN && index <= ns);
    }
    for (uint32_t s = 1; s < ns; ++s) {  // move one count between two classes: the sum stays, the counts do not
      const uint64_t* row = &b.span_base[size_t(s) * 5];
      const uint64_t* nxt = &b.span_base[size_t(s + 1) * 5];
      const uint64_t* prv = &b.span_base[size_t(s - 1) * 5];
      int from = -1, to = -1;
      for (int k = 0; k < 5; ++k) {
        if (from < 0 && row[k] > prv[k]) from = k;
        else if (to < 0 && row[k] < nxt[k]) to = k;
      }
      if (from < 0 || to < 0) continue;
      Batch c = b;
      c.span_base[size_t(s) * 5 + from] -= 1, c.span_base[size_t(s) * 5 + to] += 1;
      In x(c, true, true);
      REQUIRE(run_bad(x, &what, &index) == CLG_E_INVALID_ARG && what == CLG_ENC_BAD_SPAN && index == s);
      break;
    }
  }
}

}  // namespace

int main() {
  const uint32_t sizes[] = {0, 1, 2, 7, 64, 65, 300, 1000};
  uint64_t seed = 0xEC01;
  for (uint32_t n : sizes) {
    for (int v = 0; v < 4; ++v, ++seed) {
      std::vector<uint32_t> cuts;
      if (v == 0) cuts = {0};
      if (v == 1) cuts = {0, 0, n / 3, n / 3, n / 2, n, n};  // empty spans first, in the middle and last
      if (v == 2) cuts = {0, n / 4, n / 2, n - n / 4};
      if (v == 3) {
        for (uint32_t i = 0; i < 70; ++i) cuts.push_back(uint32_t(uint64_t(i) * n / 70));
      }
      const Batch b = make(seed, n, cuts);
      check_ok(b, cuts, true, true);
      check_ok(b, cuts, false, false);
      check_errors(b, cuts);
    }
  }
  // no payload column at all when no row carries one
  {
    Batch b;
    b.pos.push_back(0);
    b.tag = {0, 1, 6, 2};
    b.order = {5}, b.timestamp = {-2}, b.rng = {7};
    b.w_rc = {3}, b.w_v1 = {0}, b.w_v0 = {9}, b.w_sub = {0}, b.w_var_len = {0};
    In x(b, false, false);
    x.in.pos = nullptr, x.in.var = nullptr;
    clg_encoded out{};
    REQUIRE(clg::ecol_build_host(&x.in, &out) == CLG_OK && out.n_bytes == 2 + 9 + 13 + 5);
  }
  // kEcolArray names clg_columns_in's thirteen arrays in the order of the struct (which is the
  // kernels' EcolIn's: the engine asserts that), with their element widths and the counts they follow
  {
    clg_columns_in in{};
    alignas(16) static const uint8_t store[16 * (clg::kEcolArrays + 1)] = {};  // array i "lies" at store + 16 * (i + 1)
    const auto at = [&](int i) { return store + 16 * (i + 1); };
    in.tag = at(0), in.order = reinterpret_cast<const int8_t*>(at(1)), in.timestamp = reinterpret_cast<const int64_t*>(at(2));
    in.rng = reinterpret_cast<const int32_t*>(at(3)), in.buffer_built = reinterpret_cast<const int32_t*>(at(4));
    in.w_rc = reinterpret_cast<const int32_t*>(at(5)), in.w_v1 = reinterpret_cast<const int64_t*>(at(6));
    in.w_var_len = reinterpret_cast<const uint32_t*>(at(7)), in.w_sub = at(8);
    in.w_v0 = reinterpret_cast<const int64_t*>(at(9)), in.w_idx = reinterpret_cast<const uint32_t*>(at(10));
    in.pos = reinterpret_cast<const uint64_t*>(at(11)), in.var = at(12);
    in.n_rec = 100, in.n_class[0] = 10, in.n_class[1] = 11, in.n_class[2] = 12, in.n_class[3] = 13, in.n_class[4] = 14, in.n_var = 99;
    const uint32_t width[clg::kEcolArrays] = {sizeof *in.tag,   sizeof *in.order, sizeof *in.timestamp, sizeof *in.rng, sizeof *in.buffer_built,
                                              sizeof *in.w_rc,  sizeof *in.w_v1,  sizeof *in.w_var_len, sizeof *in.w_sub, sizeof *in.w_v0,
                                              sizeof *in.w_idx, sizeof *in.pos,   sizeof *in.var};
    const uint64_t len[clg::kEcolArrays] = {100, 10, 11, 12, 13, 14, 14, 14, 14, 14, 14, 15, 99};
    static_assert(clg::kEcolArrays == 13 && clg::kEcolNarrowArrays == 5 && clg::kEcolPackedArrays == 12, "tag .. buffer_built | .. pos | var");
    for (int i = 0; i < clg::kEcolArrays; ++i) {
      REQUIRE(clg::ecol_in_ptr(in, i) == at(i) && clg::kEcolArray[i].at == size_t(i) * sizeof(void*));
      REQUIRE(clg::kEcolArray[i].width == width[i] && clg::ecol_array_len(in, i) == len[i]);
      REQUIRE(clg::ecol_array_bytes(in, i) == len[i] * width[i]);
      REQUIRE(clg::kEcolArray[i].needed == (i != 10 && i != 11));  // (w_idx and pos may be absent)
    }
    REQUIRE(clg::ecol_args_ok(in));
    for (int i = 0; i < clg::kEcolArrays; ++i) {  // a null array is refused where it is needed, and set() puts one back
      clg_columns_in x = in;
      clg::ecol_in_set(&x, i, nullptr);
      REQUIRE(clg::ecol_in_ptr(x, i) == nullptr && clg::ecol_args_ok(x) == !clg::kEcolArray[i].needed);
      clg::ecol_in_set(&x, i, at(i));
      REQUIRE(memcmp(&x, &in, sizeof x) == 0);
    }
  }
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
