// placement.h -- where a kernel reads or writes a caller's arrays, decided once for every entry
// point of the columns family.  A device pointer is used as it is.  Registered host memory
// (CLG_MEM_MAPPED) is used through its device address when one registered range holds the whole
// array.  Everything else gets a slot in an engine staging buffer at 16-byte-aligned offsets, and
// the engine copies it in (inputs) or out (outputs).  The policy says what becomes of a
// registered-kind array that the registry does not hold whole:
//   stage_unless_device   nothing is looked up: all that is not device memory is staged
//   stage_if_unresolved   all the arrays are staged, as host memory is
//   reject_unresolved     the call is refused (host memory is still staged)
// Host-only, no HIP, no allocation, at most kPlaceMax arrays: the registry is a function pointer,
// and tests/placement_host.cpp passes a fake one.
#pragma once
#include <cstddef>
#include <cstdint>

namespace clg {

constexpr int kPlaceMax = 13;
// The memory kinds, numbered as CLG_MEM_* in clonos_engine.h (the engine asserts it).
enum : uint32_t { kPlaceHost = 0, kPlaceDevice = 1, kPlaceMapped = 2 };
inline bool mem_kind_ok(uint32_t kind) { return kind <= kPlaceMapped; }

enum class PlacePolicy { stage_unless_device, stage_if_unresolved, reject_unresolved };
enum class PlaceVerdict { in_place, staged, not_registered, misaligned };

struct PlaceSpec {
  const void* p;   // the caller's array (null: absent)
  uint64_t bytes;  // its length (0: empty)
  uint32_t elem;   // its element size, for the alignment check
};
// The device address of registered host memory [p, p + bytes), 0 when no one range holds it all.
using PlaceLookup = uintptr_t (*)(const void* p, uint64_t bytes);

struct Placement {
  PlaceVerdict verdict = PlaceVerdict::in_place;
  int bad = -1;                    // not_registered, misaligned: the offending array
  uintptr_t dev[kPlaceMax] = {};   // in_place: what the kernel uses; staged: set by bind()
  size_t off[kPlaceMax + 1] = {};  // every array's slot in the staging buffer; off[n] == total
  size_t total = 0;

  bool staged() const { return verdict == PlaceVerdict::staged; }
  // staged: the arrays' slots in the staging buffer at `base` (an absent array stays null)
  void bind(const PlaceSpec* s, int n, void* base) {
    for (int i = 0; i < n; ++i) dev[i] = s[i].p ? reinterpret_cast<uintptr_t>(base) + off[i] : 0;
  }
  template <class T> T* at(int i) const { return reinterpret_cast<T*>(dev[i]); }
};

// Slots of n arrays of bytes[i] each, one behind the other at 16-byte-aligned offsets: off[i] is
// array i's, off[n] the end (returned).  Also the layout of pure engine scratch.
inline size_t place_layout(const uint64_t* bytes, int n, size_t* off) {
  off[0] = 0;
  for (int i = 0; i < n; ++i) off[i + 1] = (off[i] + size_t(bytes[i]) + 15) & ~size_t(15);
  return off[n];
}
// N pieces of one scratch buffer at `base`, their offsets place_layout's: at<T>(i) is piece i's address.
template <int N>
struct Carve {
  size_t off[N + 1] = {};
  uint8_t* base = nullptr;
  template <class T> T* at(int i) const { return reinterpret_cast<T*>(base + off[i]); }
};

// Absent and empty arrays are neither looked up nor checked for alignment; in place they keep
// the caller's pointer.  Alignment is checked only where the kernel touches the caller's memory,
// that is in place: staged memory is only copied.
inline Placement place(const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, PlaceLookup lookup) {
  Placement pl;
  uint64_t bytes[kPlaceMax];
  for (int i = 0; i < n; ++i) {
    bytes[i] = s[i].p ? s[i].bytes : 0;
    pl.dev[i] = reinterpret_cast<uintptr_t>(s[i].p);
  }
  pl.total = place_layout(bytes, n, pl.off);
  bool stage = kind != kPlaceDevice;
  if (kind == kPlaceMapped && policy != PlacePolicy::stage_unless_device) {
    int i = 0;
    while (i < n && (!bytes[i] || (pl.dev[i] = lookup(s[i].p, s[i].bytes)) != 0)) ++i;
    stage = i < n;
    if (stage && policy == PlacePolicy::reject_unresolved) return pl.verdict = PlaceVerdict::not_registered, pl.bad = i, pl;
  }
  for (int i = 0; i < n && !stage; ++i)
    if (bytes[i] && reinterpret_cast<uintptr_t>(s[i].p) % s[i].elem) return pl.verdict = PlaceVerdict::misaligned, pl.bad = i, pl;
  if (!stage) return pl;
  pl.verdict = PlaceVerdict::staged;
  for (int i = 0; i < n; ++i) pl.dev[i] = 0;
  return pl;
}

}  // namespace clg
