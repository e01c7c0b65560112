// Which hnsw_search_kernel<kIP, kChunks, kMode, kSpace> instantiations exist, and which of them a
// search gets.  Host only, no HIP: capi.cpp plans a launch from the variant chosen here,
// search_kernels.hip expands the same list into the kernel pointers, and the CPU tests read both
// through alaya_search_variant / alaya_search_variant_at.
#pragma once
#include <cstddef>
#include <cstdint>

namespace alaya_amd {

// kMode bits of the search kernel.
// kModeStamp: diagnostic build that accumulates s_memtime cycles per phase into p.stamps (nq x 8):
// [0] init + overlay descent, [1] pop, [2] adjacency load + visited set, [3] distances, [4] merge,
// [5] expansions after the visited table spilled, [6] whole query, [7] prefetch hits;
// kModeCheck: the spill-table prefetch check (ALAYA_SPILL_FLAGS bit 8: every bucket read one
// expansion ahead is compared with a re-read at its use, and a stale one marks the query's counters);
// kModeHelp: distance helpers (SearchParams::help): a wave with no query left computes the distances
// of a sibling's next expansion into a memo the sibling reads (help_siblings);
// kModeTwoWaves: two waves per SIMD for wide f32 rows (one row per lane group, SearchParams::two_waves);
// kModeScreen: the candidate screen on a low-precision row copy (wide f32 L2 rows); which copy --
// f16 rows or 8-bit records -- is SearchParams::screen at run time, not a variant.
constexpr int kModeStamp = 1;
constexpr int kModeCheck = 2;
constexpr int kModeHelp = 4;
constexpr int kModeTwoWaves = 8;
constexpr int kModeScreen = 16;

// Every variant, one row each: X(space, chunks, mode, metrics).  space = SearchParams::sq8_order
// (0 = f32 rows, 1 = AVX2-order SQ8, 2 = AVX-512-order SQ8); chunks = dim / 32, 0 = the runtime-d
// kernel; metrics = both (L2 and IP) or l2.  A new kernel is a new row here and nothing else.  The
// resolver does not read the order of the rows; it is the order of the kernels in the code object.
// Why these: helpers for the small-row f32 kernels (d = 128 / 256, latency-bound) and the
// AVX-512-order SQ8 kernels; two waves and the screen for the wide f32 rows (bandwidth-bound; IP has
// no proven screening bound); stamps where tools/profile_phases.py profiles; the prefetch check for
// config 5's d = 768 / 960.
#define ALAYA_SEARCH_VARIANTS(X)                                                              \
  X(2, 24, 5, both) X(2, 24, 1, both) X(2, 24, 2, both) X(2, 30, 2, both)                     \
  X(2, 4, 4, both) X(2, 24, 4, both) X(2, 30, 4, both)                                        \
  X(2, 4, 0, both) X(2, 24, 0, both) X(2, 30, 0, both) X(2, 0, 0, both)                       \
  X(1, 24, 1, both)                                                                           \
  X(1, 4, 0, both) X(1, 24, 0, both) X(1, 30, 0, both) X(1, 0, 0, both)                       \
  X(0, 24, 24, l2) X(0, 30, 24, l2)                                                           \
  X(0, 16, 16, l2) X(0, 24, 16, l2) X(0, 30, 16, l2) X(0, 32, 16, l2)                         \
  X(0, 4, 5, both) X(0, 30, 1, both) X(0, 4, 1, both) X(0, 0, 1, both)                        \
  X(0, 4, 4, both) X(0, 8, 4, both)                                                           \
  X(0, 24, 8, both) X(0, 30, 8, both)                                                         \
  X(0, 4, 0, both) X(0, 8, 0, both) X(0, 16, 0, both) X(0, 24, 0, both) X(0, 30, 0, both)     \
  X(0, 32, 0, both) X(0, 0, 0, both)

struct SearchVariant {
  int space;
  int chunks;
  int mode;
  bool l2_only;
};

#define ALAYA_L2_ONLY_both false
#define ALAYA_L2_ONLY_l2 true
#define ALAYA_VARIANT_ROW(S, C, M, METRICS) {S, C, M, ALAYA_L2_ONLY_##METRICS},
inline constexpr SearchVariant kSearchVariants[] = {ALAYA_SEARCH_VARIANTS(ALAYA_VARIANT_ROW)};
#undef ALAYA_VARIANT_ROW
constexpr size_t kNumSearchVariants = sizeof(kSearchVariants) / sizeof(kSearchVariants[0]);

// The compile-time width of a row, 0 = none (the runtime-d kernel).
constexpr int search_chunks(uint32_t dim, bool generic) {
  return (!generic && dim % 32 == 0) ? static_cast<int>(dim / 32) : 0;
}

// Whether a search of this shape has a kernel with this feature (a kMode bit) at all.
constexpr bool search_has(int bit, uint32_t dim, int sq8_order, bool generic, bool ip) {
  for (const SearchVariant &v : kSearchVariants)
    if (v.space == sq8_order && v.chunks == search_chunks(dim, generic) && (v.mode & bit) != 0 && !(v.l2_only && ip))
      return true;
  return false;
}
constexpr bool search_has_helpers(uint32_t dim, int sq8_order, bool generic) {
  return search_has(kModeHelp, dim, sq8_order, generic, false);
}
constexpr bool search_has_two_waves(uint32_t dim, int sq8_order, bool generic) {
  return search_has(kModeTwoWaves, dim, sq8_order, generic, false);
}
constexpr bool search_has_screen(uint32_t dim, int sq8_order, bool generic, bool ip) {
  return search_has(kModeScreen, dim, sq8_order, generic, ip);
}

// What a search asks for: its shape and the features (kMode bits) that policy wants.
struct SearchRequest {
  uint32_t dim;
  bool ip;
  int sq8_order;
  bool generic;  // the generic element order of f32 rows: the runtime-d kernel (SQ8 codes ignore it)
  int want;
};

// Where no variant has everything wanted, features are given up from the back of this list: a
// variant with an earlier feature beats any variant without it.
constexpr int kFeaturePriority[] = {kModeScreen, kModeStamp, kModeCheck, kModeHelp, kModeTwoWaves};

constexpr int search_mode_rank(int mode) {
  int rank = 0;
  for (int bit : kFeaturePriority) rank = 2 * rank + ((mode & bit) != 0 ? 1 : 0);
  return rank;
}

// The variant a request gets: of the variants of its space and metric with no feature it did not
// ask for, at its compile-time width or runtime-d, the one of the highest rank; at equal rank the
// compile-time width.  The screen is only for a search that wants neither stamps nor helpers, whether
// or not its width has kernels with those.  Every space has the plain runtime-d kernel, so there is
// always a variant; what was wanted and is not in its mode was dropped, and the caller plans for
// the mode it got.
constexpr const SearchVariant &resolve_search_variant(const SearchRequest &r) {
  const int want = (r.want & (kModeStamp | kModeHelp)) != 0 ? r.want & ~kModeScreen : r.want;
  const int chunks = search_chunks(r.dim, r.generic && r.sq8_order == 0);
  const SearchVariant *best = nullptr;
  int best_rank = -1;
  for (const SearchVariant &v : kSearchVariants) {
    if (v.space != r.sq8_order || (v.mode & ~want) != 0 || (v.l2_only && r.ip)) continue;
    if (v.chunks != chunks && v.chunks != 0) continue;
    const int rank = 2 * search_mode_rank(v.mode) + (v.chunks == chunks ? 1 : 0);
    if (rank > best_rank) {
      best = &v;
      best_rank = rank;
    }
  }
  return *best;
}

}  // namespace alaya_amd
