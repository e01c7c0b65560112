// Launch interface between the C-ABI layer (capi.cpp) and the device code (search_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "search_variants.h"

namespace alaya_amd {

// Everything one search launch reads or writes.  All pointers are device pointers.
struct SearchParams {
  // base rows (RawSpace storage): n rows of `stride` floats, first `dim` used, zero padded
  const float *base;
  uint64_t n;
  uint32_t dim;
  uint32_t stride;        // multiple of 32 floats (128 B rows, 16 B aligned float4 loads)
  const uint32_t *valid;  // SequentialStorage validity bitmap as 32-bit words; nullptr = all valid
  bool ip;                // IP / COS (negated inner product) vs L2
  bool generic;           // non-float DataType: generic l2_sqr<T>/ip_sqr<T> order (one accumulator,
                          // elements in order; distance_l2.ipp:735-741), not the AVX2 float order
  // level-0 adjacency (Graph), n x R, -1 padded
  const uint32_t *l0;
  uint32_t R;
  bool dedup_edges;       // some row repeats an id: drop later occurrences in-kernel
  // overlay (OverlayGraph); levels == nullptr -> NSG-style entry points
  const uint32_t *levels;
  const uint64_t *upper_off;
  const uint32_t *upper_edges;
  uint32_t upper_R;
  uint32_t ep;
  const uint32_t *eps;
  uint32_t n_eps;
  // batch
  const float *queries;   // nq rows of q_stride floats
  uint64_t nq;
  uint32_t q_stride;
  uint32_t k;
  uint32_t ef;
  uint32_t *out_ids;      // nq x k
  float *out_dists;       // nq x k (nullable)
  uint32_t *out_counters; // nq x 4 (n_dist, n_expand, n_dist_upper, n_hops_upper), nullable
  uint32_t fill_id;       // id written for result slots past the pool (0 = reference behaviour, with
                          // distance 0.0; 0xffffffff = empty slot, with distance FLT_MAX)
  // scratch
  uint32_t *work_counter; // zeroed before each launch
  uint32_t *overflow_bits;// grid x ceil(n/32) words: visited-set spill area, all zero between queries
  uint32_t *dirty_words;  // slots x dirty_cap: per-slot list of the spill-area words a query set
  uint32_t dirty_cap;
  uint32_t wave_lds;      // bytes of one wave's LDS region (search_wave_lds_bytes)
  uint32_t hash_log2;     // LDS visited table = 1 << hash_log2 slots
  // visited-table layout: kVisWide = 32-bit id slots; otherwise 16-bit compact slots holding
  // (probe distance, low vis_rbits bits of a vis_lbits-bit bijective hash) -- exact either way
  uint32_t vis_rbits;
  uint32_t vis_lbits;
  uint32_t vis_max_disp;  // compact: largest probe distance an entry may sit at (<= 0xffff >> rbits - 1)
  uint32_t vis_limit;     // LDS table entries before a query spills to the second level (0 = the
                          // layout's default: half the slots wide, 11/16 compact); <= slots - 64
  // Spill table (stab_log2 != 0): the second level is a per-slot hash table of 2^stab_log2 16-bit
  // entries in buckets of 8 (16 B), all zero between queries, instead of the N-bit bitset; the bitset
  // stays as a third level for the (rare) ids whose home bucket is full.  An entry is 1 + the low
  // stab_rbits bits of the vis_lbits-bit bijective hash, whose top bits are the bucket.
  uint16_t *spill_table;  // slots x 2^stab_log2 entries
  uint32_t stab_log2;
  uint32_t stab_rbits;    // <= 15
  uint32_t spill_flags;   // diagnostics (ALAYA_SPILL_FLAGS): bit 0 = no second-level prefetch, bit 2 =
                          // prefetch after the rows land, bit 8 = the prefetch-check kernel (kDiag 2)
  uint64_t *stamps;       // nullable: diagnostic per-phase cycle counts, nq x 8
  // SQ8 search space (SQ8Space, space/sq8_space.hpp): traversal distances on uint8 codes
  int sq8_order;          // 0 = f32 RawSpace search; 2 = AVX-512 SQ8 order; 1 = AVX2 SQ8 order
  const uint8_t *codes;   // n rows of code_stride bytes (16 B aligned)
  uint32_t code_stride;
  const float *sq_min;    // per-dimension min / max of SQ8Quantizer (sq8.hpp:99-113)
  const float *sq_max;
  // distance helpers (search_has_helpers): 1 = a wave with no query left computes its workgroup
  // siblings' next distances into an LDS memo (kHelpBoardBytes after the wave regions); help_flags
  // are diagnostics (ALAYA_HELP_FLAGS bit 0 = no visited hint: helpers compute every claimed row;
  // bit 1 = the hint in the f32 kernels too -- by default only the SQ8 kernels use it)
  uint32_t help;
  uint32_t help_flags;
  uint32_t memo_off;      // byte offset of a helper's memo in its wave region (0: the query vector)
  uint32_t two_waves;     // 1 = the wide-row f32 kernel at two waves per SIMD (one row per lane group):
                          // twice the resident searchers, each with half the rows in flight (0 in a scouted
                          // launch, which runs that kernel for its registers: its second wave is the scout)
  uint32_t *help_stats;   // nullable: per searcher, (fresh distances it took from a memo, expansions
                          // with every fresh distance from the memo, rows it computed as a helper)
  // Candidate screen (search_has_screen; kModeScreen): once the pool is full, an expansion's fresh
  // candidates are first measured on a low-precision copy of their rows, and only those whose proven
  // lower bound (screen_bound.h) is below the pool's worst distance read their f32 row.
  uint32_t screen;             // the screening kernel's copy: 0 = none, 1 = f16, 2 = 8-bit records,
                               // 3 = the same records under integer dot products with the query's codes
  const uint16_t *screen_rows; // f16: n rows of `stride` f16 values (stride * 2 bytes, a multiple of 64)
  const float *screen_err;     // f16: per row, >= ||x - f16(x)||_2; +inf = never screened out
  const uint8_t *screen_u8;    // 8-bit: n records of screen_u8_record_bytes(stride) bytes (screen_bound.h):
                               // {e_row, lo, scale, 0} and `stride` codes
  uint32_t *screen_stats;      // per searcher: (candidates screened, candidates screened out)
  // Scout (the two-waves screening kernels, screen == 3; search kernel "Scout"): every searcher wave has
  // a second wave in its workgroup that computes the integer screen's bounds for the nodes the searcher
  // will probably pop next into an LDS memo (kScoutBoardBytes after the wave regions).  Bits:
  // kScoutOn; kScoutVerify = on a memo hit the searcher also computes its own bounds and counts the
  // ones that differ; kScoutMiss = diagnostics: the scout answers only the request for the pop after
  // the next, under a tag no lookup matches (every expansion falls back).
  uint32_t scout;
  uint32_t *scout_stats;       // per searcher: (expansions screened, memo hits, records the scout read,
                               // verify mismatches)
  // What the scout is asked and when it gives a node up (wave-uniform, 0 when scout == 0; hints both:
  // no bound, result or counter depends on a bit).  kScoutEarly = the searcher names the likely
  // retarget -- the screen's survivor with the smallest bound, if that bound is below the first
  // unchecked entry's distance -- right after the screen, an exact pass and a merge before on_next can;
  // kScoutRecheck = the scout looks at the requests again once a node's adjacency row has arrived and
  // drops a node that is in neither.
  uint32_t scout_policy;
  uint32_t *scout_policy_stats;  // per searcher: (early requests, those on_next confirmed, nodes the
                                 // scout dropped at the re-check)
};
constexpr uint32_t kScoutOn = 1, kScoutVerify = 2, kScoutMiss = 4;
constexpr uint32_t kScoutEarly = 1, kScoutRecheck = 2;  // SearchParams::scout_policy
constexpr uint32_t kScoutSlots = 3;   // requests, and memo rows, per searcher
constexpr uint32_t kScoutR = 32;      // adjacency positions per memo row: one pass of the integer screen
// one searcher's board: kScoutSlots memo rows of kScoutR bounds, their tags, the requests, the state
// word and the searcher's three counters
constexpr size_t kScoutBoardBytes = kScoutSlots * (kScoutR * 4 + 8 + 4) + 20;

// The filtered search's own arguments (filtered_search_kernel's second argument: SearchParams keeps
// its layout).  All pointers are device pointers.
struct FilterParams {
  const uint32_t *allow;          // n_masks x mask_words words; bit i of word i / 32 = row i (the validity
                                  // bitmap's layout)
  const uint32_t *mask_of_query;  // nq indices below n_masks; nullptr = every query uses mask 0
  uint32_t mask_words;            // ceil(n / 32)
  uint32_t k;                     // the result pool's capacity (= SearchParams::k)
  uint32_t result_off;            // byte offset of the result pool in a wave's LDS region (past the
                                  // visited table: SearchParams::wave_lds - filter_result_lds_bytes(k))
};

// What the through search (filtered_hop_search_kernel) takes beyond SearchParams and FilterParams: its
// third argument.
struct HopParams {
  uint32_t *n_through;  // nq: rows stepped through per query (nullable)
};

// The range search's own arguments (range_search_kernel's third argument; range_sort_kernel's only
// one).  All pointers are device pointers.  The search kernel appends query i's hits, in arrival order,
// to slots [i * cap, i * cap + min(counts[i], cap)) of append_ids / append_dists and leaves the other
// slots unwritten; the sort kernel reads those and writes out_ids / out_dists.
struct RangeParams {
  const float *radii;    // nq: a hit has d <= radii[i]
  uint32_t cap;          // stored rows per query (1 .. kRangeMaxCap)
  uint32_t *append_ids;  // nq x cap
  float *append_dists;   // nq x cap
  uint32_t *counts;      // nq: hits per query, not capped
  uint32_t *out_ids;     // nq x cap: the stored rows by (distance, id), then (kEmpty, FLT_MAX)
  float *out_dists;      // nq x cap
};
constexpr uint32_t kRangeMaxCap = 4096;

// What the radius-mode range search (range_more_search_kernel) takes beyond range_search_kernel's
// arguments: its fourth argument.  The kernel stores the first min(frontier count, cap) rows that join
// query i's frontier in slots [i * cap, ...) of frontier_ids, and reads them back itself.
struct RangeMoreParams {
  uint32_t *frontier_ids;  // nq x cap
  uint32_t cap;            // stored frontier rows per query (1 .. kRangeMaxFrontier)
  uint32_t *more;          // nq x 2 (rows that joined the frontier, not capped; distances of phase 2), nullable
};
constexpr uint32_t kRangeMaxFrontier = 16384;

// PyIndex::rerank inputs (python/include/index.hpp:450-488).  Per query the kernel rescores
// search_ids[0 .. n_take) (row stride n_src; kEmpty entries are skipped) plus `zeros` entries of id 0
// -- the reference's res_pool slots [k, ef) that batch_search leaves zero (index.hpp:301) -- and
// returns the k smallest pair<dist, id>.
//   reference mode:  n_take = min(k, ef), zeros = ef - k, fill_id = 0
//   corrected mode:  n_take = ef (the whole pool, kEmpty past it), zeros = 0, fill_id = 0
//   shard mode:      n_take = min(k, ef); zeros = ef - k only on the shard that holds global row 0,
//                    else 0; fill_id = kEmpty (see alaya_index_shard_search_sq8_device)
struct RerankParams {
  const uint32_t *search_ids;  // nq x n_src ids written by the SQ8 search
  uint32_t k;
  uint32_t n_src;              // ids per query row of search_ids
  uint32_t n_take;             // ids rescored per query (<= n_src)
  uint32_t zeros;              // multiplicity of the extra id-0 entry (0 = none)
  uint32_t fill_id;            // output slots without a candidate: 0 -> (0, 0.0), kEmpty -> (kEmpty, FLT_MAX)
  uint32_t *out_ids;           // nq x k
  float *out_dists;            // nq x k (nullable)
};

constexpr uint32_t kVisWide = 0xffffffffu;
constexpr size_t kHelpBoardBytes = 256;  // the helpers' request board (search kernel, kModeHelp)
#ifndef ALAYA_HELP_DEPTH
#define ALAYA_HELP_DEPTH 1
#endif
constexpr size_t kHelpMemoSlots = ALAYA_HELP_DEPTH + 1;  // memo rows (requests) per searcher
constexpr uint32_t kStabBucket = 8;  // spill-table entries per bucket (16 B: one prefetch per lane)
// bytes of the LDS visited table / of one wave's LDS region / of a workgroup's shared region
// (SQ8: the quantizer's per-dimension scale and min); a workgroup of W waves takes
// shared + W * wave bytes
inline size_t visited_table_bytes(uint32_t hash_log2, bool compact) {
  return (static_cast<size_t>(compact ? 2 : 4)) << hash_log2;
}
size_t search_wave_lds_bytes(uint32_t stride, uint32_t ef, uint32_t hash_log2, bool compact = false,
                             int sq8_order = 0);
// bytes of a wave's query region: stride f32 terms, or the query's codes (AVX-512-order SQ8 kernels
// built with ALAYA_SQ8_QCODES)
size_t search_query_lds_bytes(uint32_t stride, int sq8_order);
__host__ __device__ inline size_t search_shared_lds_bytes(uint32_t stride, bool sq8) {
  return sq8 ? 2 * static_cast<size_t>(stride) * 4 : 0;
}
// rerank: p.base/p.queries are the raw f32 rows and the (normalised) f32 queries
hipError_t launch_rerank(const SearchParams &p, const RerankParams &r, hipStream_t stream);
// resident workgroups per CU of variant `v`'s kernel (search_variants.h) for the metric
hipError_t search_occupancy(const SearchVariant &v, bool ip, int waves, size_t lds, int *blocks_per_cu);
// The screening copy of rows [first, first + count): out_rows[r] = f16(base[r]) (stride halfs per
// row) and out_err[r] >= ||base[r] - f16(base[r])||_2, +inf for a row with an element that is not
// finite in f16.
hipError_t launch_screen_rows(const float *base, uint64_t first, uint64_t count, uint32_t stride,
                              uint16_t *out_rows, float *out_err, hipStream_t stream);
// The 8-bit screening copy of rows [first, first + count): record r of out_recs (screen_bound.h:
// screen_u8_record_bytes(stride) bytes each) = {e_row, lo, scale, 0} and the row's codes, with
// e_row >= ||base[r] - y||_2 for y_j = screen_u8_value(code_j, lo, scale); +inf for a row that is not
// finite.
hipError_t launch_screen_rows_u8(const float *base, uint64_t first, uint64_t count, uint32_t stride,
                                 uint8_t *out_recs, hipStream_t stream);
// launches variant `v`'s kernel: the one resolve_search_variant chose and p.help / p.two_waves /
// p.screen / the LDS layout were planned for
hipError_t launch_search(const SearchVariant &v, const SearchParams &p, int grid, int waves, size_t lds,
                         hipStream_t stream);
// Filtered search (filtered_search_kernel; f32 rows): bytes of a wave's result pool (k + 1 distances and
// ids), the kernel of the shape's resident workgroups per CU, and its launch.  p is planned as the
// plain (mode 0) search of the shape, with the result pool's bytes at the end of p.wave_lds.
size_t filter_result_lds_bytes(uint32_t k);
hipError_t filtered_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu);
hipError_t launch_filtered_search(const SearchParams &p, const FilterParams &f, int grid, int waves, size_t lds,
                                  hipStream_t stream);
// The through search (filtered_hop_search_kernel; f32 rows): the filtered search's plan and LDS layout, its
// own kernel's resident workgroups per CU, and its launch.
hipError_t filtered_hop_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu);
hipError_t launch_filtered_hop_search(const SearchParams &p, const FilterParams &f, const HopParams &h, int grid, int waves,
                                      size_t lds, hipStream_t stream);
// Range search (range_search_kernel; f32 rows): p is planned as the plain (mode 0) search of the shape,
// with no result pool (p.k = 0: the kernel writes no result rows, only r.counts, the append buffers and
// p.out_counters); f.allow == nullptr = no mask.  launch_range_sort (range_sort_kernel) then orders
// every query's stored rows: one workgroup per query, 8 bytes of LDS per slot of the cap's power of two.
hipError_t range_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu);
hipError_t launch_range_search(const SearchParams &p, const FilterParams &f, const RangeParams &r, int grid, int waves,
                               size_t lds, hipStream_t stream);
hipError_t launch_range_sort(const RangeParams &r, uint64_t nq, hipStream_t stream);
// The radius-mode range search (range_more_search_kernel): range_search_kernel's plan and arguments, its own
// kernel's resident workgroups per CU, and its launch; launch_range_sort follows as above.
hipError_t range_more_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu);
hipError_t launch_range_more_search(const SearchParams &p, const FilterParams &f, const RangeParams &r,
                                    const RangeMoreParams &m, int grid, int waves, size_t lds, hipStream_t stream);
// Filtered search of SQ8 codes (filtered_sq8_search_kernel): f.k = p.k = m, the candidate pool's capacity
// (filter_result_lds_bytes(m) at the end of p.wave_lds); p is planned as the plain (mode 0) SQ8 search of
// the shape and p.out_ids receives nq x m candidate ids, kEmpty in empty slots, for launch_rerank.
hipError_t filtered_sq8_search_occupancy(uint32_t dim, int sq8_order, bool ip, int waves, size_t lds,
                                         int *blocks_per_cu);
hipError_t launch_filtered_sq8_search(const SearchParams &p, const FilterParams &f, int grid, int waves, size_t lds,
                                      hipStream_t stream);
// Range search of SQ8 codes (range_sq8_search_kernel): p is planned as the plain (mode 0) SQ8 search of the
// shape with no result pool (p.k = 0); r.radii are the code radii, r.counts receives the candidate counts
// and the append buffers the first r.cap (id, code distance) candidates per query; f.allow == nullptr = no
// mask.  launch_range_rerank (range_rerank_kernel) then takes p.base / p.queries as the f32 rows and the
// rerank queries, r.radii as the exact radii and r.counts as those candidate counts: it overwrites the
// stored code distances with exact ones, turns a candidate past its radius into the sort's pad and adds the
// hits to hits[i], which the caller zeroes on the stream first.  launch_range_sort follows with the same r.
hipError_t range_sq8_search_occupancy(uint32_t dim, int sq8_order, bool ip, int waves, size_t lds, int *blocks_per_cu);
hipError_t launch_range_sq8_search(const SearchParams &p, const FilterParams &f, const RangeParams &r, int grid, int waves,
                                   size_t lds, hipStream_t stream);
hipError_t launch_range_rerank(const SearchParams &p, const RangeParams &r, uint32_t *hits, hipStream_t stream);
// out[q * n + i] = dist(queries[q], base[ids[i]]) for q < nq (bit-exact device distance)
hipError_t launch_row_distances(const SearchParams &p, const uint32_t *ids, uint32_t n,
                                uint32_t nq, float *out, hipStream_t stream);

// streaming read of `bytes` (multiple of 16) for the measured-bandwidth calibration
hipError_t launch_stream_read(const void *buf, uint64_t bytes, int grid, int shape, float *sink,
                              hipStream_t stream);

}  // namespace alaya_amd
