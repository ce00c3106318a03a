// placement_host.cpp -- clonos_amd/csrc/placement.h against a fake registry of two adjacent
// ranges: every memory kind under every policy, arrays at and past a range's end and across the
// seam of the two ranges, absent, empty and misaligned arrays, and the staging layout.
// Stand-alone: g++ -std=c++17 tests/placement_host.cpp (tests/test_placement_host.py).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../clonos_amd/csrc/placement.h"

using namespace clg;

static long checks = 0;
static bool ok(const Placement& pl) { return pl.verdict == PlaceVerdict::in_place || pl.staged(); }
#define CHECK(x)                                               \
  do {                                                         \
    ++checks;                                                  \
    if (!(x)) {                                                \
      printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                 \
    }                                                          \
  } while (0)

// Host [kA, kA + kLen) maps to kDevA, host [kB, kB + kLen) to kDevB; kB == kA + kLen, so the
// ranges are adjacent in host memory and far apart on the device.
constexpr uintptr_t kA = 0x100000, kLen = 0x1000, kB = kA + kLen, kDevA = 0x7000000, kDevB = 0x9000000;
static int lookups = 0;
static uintptr_t fake_lookup(const void* p, uint64_t n) {
  ++lookups;
  const uintptr_t h = reinterpret_cast<uintptr_t>(p);
  const uintptr_t host[2] = {kA, kB}, dev[2] = {kDevA, kDevB};
  for (int r = 0; r < 2; ++r)
    if (h >= host[r] && h < host[r] + kLen && n <= host[r] + kLen - h) return dev[r] + (h - host[r]);
  return 0;
}
static const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

// offsets 16-byte aligned, increasing, non-overlapping, the total equal to the last offset
static void check_layout(const Placement& pl, const PlaceSpec* s, int n) {
  CHECK(pl.off[0] == 0 && pl.total == pl.off[n]);
  for (int i = 0; i < n; ++i) {
    const uint64_t bytes = s[i].p ? s[i].bytes : 0;
    CHECK(pl.off[i] % 16 == 0);
    CHECK(pl.off[i + 1] >= pl.off[i] + bytes && pl.off[i + 1] < pl.off[i] + bytes + 16);
  }
}

static const PlacePolicy kPolicies[3] = {PlacePolicy::stage_unless_device, PlacePolicy::stage_if_unresolved,
                                         PlacePolicy::reject_unresolved};

int main() {
  CHECK(mem_kind_ok(kPlaceHost) && mem_kind_ok(kPlaceDevice) && mem_kind_ok(kPlaceMapped) && !mem_kind_ok(3) && !mem_kind_ok(~0u));

  // ---- every kind under every policy: all arrays inside range A, then one of them outside both
  for (const PlacePolicy policy : kPolicies)
    for (int outside = 0; outside < 2; ++outside) {
      const PlaceSpec s[3] = {{at(kA), 100, 4}, {at(outside ? kB + kLen : kA + 0x200), 17, 1}, {at(kA + 0x400), 64, 8}};
      // device: as it is, never looked up
      lookups = 0;
      Placement pl = place(s, 3, kPlaceDevice, policy, fake_lookup);
      CHECK(pl.verdict == PlaceVerdict::in_place && ok(pl) && !pl.staged() && lookups == 0 && pl.bad == -1);
      for (int i = 0; i < 3; ++i) CHECK(pl.dev[i] == reinterpret_cast<uintptr_t>(s[i].p));
      check_layout(pl, s, 3);
      // host: staged, never looked up
      pl = place(s, 3, kPlaceHost, policy, fake_lookup);
      CHECK(pl.verdict == PlaceVerdict::staged && ok(pl) && pl.staged() && lookups == 0);
      CHECK(pl.off[1] == 112 && pl.off[2] == 144 && pl.total == 208);
      check_layout(pl, s, 3);
      pl.bind(s, 3, reinterpret_cast<void*>(uintptr_t(0x5000)));
      for (int i = 0; i < 3; ++i) CHECK(pl.dev[i] == 0x5000 + pl.off[i]);
      // registered
      pl = place(s, 3, kPlaceMapped, policy, fake_lookup);
      check_layout(pl, s, 3);
      if (policy == PlacePolicy::stage_unless_device) {
        CHECK(pl.verdict == PlaceVerdict::staged && lookups == 0);
      } else if (!outside) {
        CHECK(pl.verdict == PlaceVerdict::in_place && lookups == 3);
        CHECK(pl.dev[0] == kDevA && pl.dev[1] == kDevA + 0x200 && pl.dev[2] == kDevA + 0x400);
      } else if (policy == PlacePolicy::stage_if_unresolved) {
        CHECK(pl.verdict == PlaceVerdict::staged && pl.dev[0] == 0 && pl.dev[1] == 0 && pl.dev[2] == 0);
      } else {
        CHECK(pl.verdict == PlaceVerdict::not_registered && pl.bad == 1 && !ok(pl) && !pl.staged());
      }
    }

  // ---- the ends of a range and the seam between the two
  for (const PlacePolicy policy : {PlacePolicy::stage_if_unresolved, PlacePolicy::reject_unresolved}) {
    const PlaceVerdict unresolved =
        policy == PlacePolicy::reject_unresolved ? PlaceVerdict::not_registered : PlaceVerdict::staged;
    // ending exactly at A's end, and at B's
    PlaceSpec s[2] = {{at(kA + kLen - 48), 48, 8}, {at(kB + kLen - 1), 1, 1}};
    Placement pl = place(s, 2, kPlaceMapped, policy, fake_lookup);
    CHECK(pl.verdict == PlaceVerdict::in_place && pl.dev[0] == kDevA + kLen - 48 && pl.dev[1] == kDevB + kLen - 1);
    // one byte past B's end
    s[1].bytes = 2;
    pl = place(s, 2, kPlaceMapped, policy, fake_lookup);
    CHECK(pl.verdict == unresolved && (unresolved == PlaceVerdict::staged || pl.bad == 1));
    // one byte past A's end is B's first byte: the array spans two adjacent ranges, which no one
    // device address covers
    s[1] = {at(kB), 16, 1};
    s[0].bytes = 49;
    pl = place(s, 2, kPlaceMapped, policy, fake_lookup);
    CHECK(pl.verdict == unresolved && (unresolved == PlaceVerdict::staged || pl.bad == 0));
    // the whole of A and the whole of B, as two arrays: each resolves
    s[0] = {at(kA), kLen, 16};
    s[1] = {at(kB), kLen, 16};
    pl = place(s, 2, kPlaceMapped, policy, fake_lookup);
    CHECK(pl.verdict == PlaceVerdict::in_place && pl.dev[0] == kDevA && pl.dev[1] == kDevB);
    // the whole of both as one array
    s[0].bytes = 2 * kLen;
    pl = place(s, 1, kPlaceMapped, policy, fake_lookup);
    CHECK(pl.verdict == unresolved);
    // just before A
    s[0] = {at(kA - 1), 2, 1};
    pl = place(s, 1, kPlaceMapped, policy, fake_lookup);
    CHECK(pl.verdict == unresolved);
  }

  // ---- absent and empty arrays: no lookup, no alignment check, no room in the staging buffer
  for (const PlacePolicy policy : kPolicies)
    for (const uint32_t kind : {kPlaceHost, kPlaceDevice, kPlaceMapped}) {
      // (0xDEAD01 lies in no range and is odd: it must be neither looked up nor checked)
      const PlaceSpec s[4] = {{nullptr, 0, 8}, {at(0xDEAD01), 0, 8}, {nullptr, 40, 4}, {at(kA + 8), 24, 8}};
      lookups = 0;
      Placement pl = place(s, 4, kind, policy, fake_lookup);
      const bool looks = kind == kPlaceMapped && policy != PlacePolicy::stage_unless_device;
      CHECK(ok(pl) && lookups == (looks ? 1 : 0));
      CHECK(pl.off[1] == 0 && pl.off[2] == 0 && pl.off[3] == 0 && pl.total == 32);
      check_layout(pl, s, 4);
      if (pl.staged()) {
        pl.bind(s, 4, reinterpret_cast<void*>(uintptr_t(0x6000)));
        // (a staged empty array gets a valid address, an absent one stays null)
        CHECK(pl.dev[0] == 0 && pl.dev[1] == 0x6000 && pl.dev[2] == 0 && pl.dev[3] == 0x6000);
      } else {
        CHECK(pl.dev[0] == 0 && pl.dev[1] == 0xDEAD01 && pl.dev[2] == 0);
        CHECK(pl.dev[3] == (looks ? kDevA + 8 : kA + 8));
      }
    }
  {
    Placement pl = place(nullptr, 0, kPlaceMapped, PlacePolicy::reject_unresolved, fake_lookup);
    CHECK(pl.verdict == PlaceVerdict::in_place && pl.total == 0);
    pl = place(nullptr, 0, kPlaceHost, PlacePolicy::reject_unresolved, fake_lookup);
    CHECK(pl.verdict == PlaceVerdict::staged && pl.total == 0);
  }

  // ---- a misaligned array reports its own index where the arrays are used in place; staged
  // memory is only copied, so it is never misaligned
  for (const PlacePolicy policy : kPolicies)
    for (int bad = 0; bad < 3; ++bad) {
      PlaceSpec s[3] = {{at(kA), 8, 8}, {at(kA + 0x100), 8, 4}, {at(kA + 0x200), 32, 16}};
      s[bad].p = at(reinterpret_cast<uintptr_t>(s[bad].p) + s[bad].elem / 2);
      lookups = 0;
      Placement pl = place(s, 3, kPlaceDevice, policy, fake_lookup);
      CHECK(pl.verdict == PlaceVerdict::misaligned && pl.bad == bad && !ok(pl) && lookups == 0);
      pl = place(s, 3, kPlaceMapped, policy, fake_lookup);
      if (policy == PlacePolicy::stage_unless_device)
        CHECK(pl.verdict == PlaceVerdict::staged && lookups == 0);
      else
        CHECK(pl.verdict == PlaceVerdict::misaligned && pl.bad == bad && !ok(pl) && lookups == 3);
      CHECK(place(s, 3, kPlaceHost, policy, fake_lookup).verdict == PlaceVerdict::staged);
      // misaligned and not registered whole: staged (or refused), not misaligned
      PlaceSpec u[2] = {s[bad], {at(kB + kLen - 4), 8, 4}};
      pl = place(u, 2, kPlaceMapped, policy, fake_lookup);
      if (policy == PlacePolicy::reject_unresolved)
        CHECK(pl.verdict == PlaceVerdict::not_registered && pl.bad == 1);
      else
        CHECK(pl.verdict == PlaceVerdict::staged);
      s[bad].bytes = 0;  // (an empty array is let be)
      CHECK(place(s, 3, kPlaceDevice, policy, fake_lookup).verdict == PlaceVerdict::in_place);
    }

  // ---- the layout at every length around a slot's size, for kPlaceMax arrays
  for (uint64_t len = 0; len <= 49; ++len) {
    PlaceSpec s[kPlaceMax];
    uint64_t bytes[kPlaceMax];
    for (int i = 0; i < kPlaceMax; ++i) {
      bytes[i] = (len + 7 * i) % 50;
      s[i] = {at(0x1000 + 0x100 * i), bytes[i], 1};
    }
    const Placement pl = place(s, kPlaceMax, kPlaceHost, PlacePolicy::stage_if_unresolved, fake_lookup);
    check_layout(pl, s, kPlaceMax);
    size_t off[kPlaceMax + 1];
    CHECK(place_layout(bytes, kPlaceMax, off) == pl.total);
    for (int i = 0; i <= kPlaceMax; ++i) CHECK(off[i] == pl.off[i]);
    // the typed carve of pure scratch: place_layout's offsets from its base
    Carve<kPlaceMax> cv;
    CHECK(cv.base == nullptr && place_layout(bytes, kPlaceMax, cv.off) == pl.total);
    alignas(16) static uint8_t scratch[kPlaceMax * 64 + 16];
    CHECK(pl.total + 16 <= sizeof scratch);
    cv.base = scratch;
    for (int i = 0; i <= kPlaceMax; ++i) CHECK(cv.off[i] == off[i]);
    for (int i = 0; i < kPlaceMax; ++i)
      CHECK(cv.at<uint8_t>(i) == scratch + off[i] && reinterpret_cast<uint8_t*>(cv.at<uint64_t>(i)) == scratch + off[i]);
  }

  printf("ok %ld\n", checks);
  return 0;
}
