// What the two exact row scans share on the host: the exact filtered k-NN (flat_filtered_kernels.hip) and the
// exact range search (flat_range_kernels.hip) run the same distance pass (exact_scan_device.h) over the same
// grid -- row chunks (ranges of an ascending id list) x query tiles -- so the shape constants, the tile
// choice, the chunk sizing, the split of a batch over launches and the launch checks are written once here.
// What a scan keeps per (chunk, query) pair, and the cap on it, stays with that scan.  The second half does the
// same for the three MFMA scans (flat_mfma_scan.h): their shape constants, chunk planner and launch check.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace alaya_amd {

constexpr uint32_t kScanPassRows = 32;    // rows one wave takes per pass: 8 lane groups x 4 rows
constexpr uint32_t kScanWaveQueries = 4;  // queries of one wave (its register sub-tile)
constexpr uint32_t kScanMaxTile = 16;     // queries per workgroup: 4, 8 or 16 (1, 2 or 4 waves)
constexpr size_t kScanLdsMax = 160 * 1024;

// Query tile: 16 (four waves share each row read), smaller for a handful of queries, and smaller where two
// workgroups would no longer fit a CU's LDS -- the second one hides the row loads' latency.  lds_at(tile): the
// LDS bytes of one workgroup.  0: the shape does not fit.
template <class LdsAt>
uint32_t scan_tile(uint64_t nq, LdsAt lds_at) {
  uint32_t tile = nq <= 4 ? 4 : (nq <= 8 ? 8 : kScanMaxTile);
  while (tile > kScanWaveQueries && lds_at(tile) > kScanLdsMax / 2) tile /= 2;
  return lds_at(tile) > kScanLdsMax ? 0 : tile;
}

inline uint64_t scan_passes(uint64_t n_ids) { return (n_ids + kScanPassRows - 1) / kScanPassRows; }

// Id-list entries per row chunk, a multiple of kScanPassRows: no more chunks than fill the CUs twice over at
// this tile -- rounded down: two workgroups are resident per CU, and a grid a little past 2 x cus would run a
// second, nearly empty round.  forced_rows: 0, or the diagnostics' rows per chunk (rounded up to whole passes).
inline uint64_t scan_chunk_rows(uint64_t n_ids, uint64_t nq, uint32_t tile, uint32_t cus, uint64_t forced_rows) {
  if (forced_rows) return scan_passes(forced_rows) * kScanPassRows;
  const uint64_t q_tiles = std::max<uint64_t>(1, (nq + tile - 1) / tile);
  const uint64_t max_chunks = std::max<uint64_t>(1, 2ull * cus / q_tiles);
  return kScanPassRows * std::max<uint64_t>(1, (scan_passes(n_ids) + max_chunks - 1) / max_chunks);
}

// Queries per scan launch, a multiple of the tile: all of them, or as many as keep chunks x queries pairs of
// pair_bytes each within `budget` (the caller sized the chunks so that one tile fits).
inline uint64_t scan_sub_queries(uint64_t nq, uint32_t tile, uint64_t chunks, uint64_t budget, uint64_t pair_bytes) {
  const uint64_t all = (std::max<uint64_t>(nq, 1) + tile - 1) / tile * tile;
  return chunks ? std::min(all, budget / (chunks * pair_bytes) / tile * tile) : all;
}

// The grid of a scan launch, or 0 for a launch that must not run: the tile is 4, 8 or 16, there are queries,
// the chunks cover n_ids exactly (the last one is not empty), and the grid is below 2^31.
inline uint32_t scan_grid(uint32_t tile, uint64_t nq, uint64_t n_ids, uint64_t chunk_rows, uint64_t chunks) {
  if (tile != 4 && tile != 8 && tile != 16) return 0;
  if (nq == 0 || chunks == 0 || chunk_rows == 0) return 0;
  if (chunks * chunk_rows < n_ids || (chunks - 1) * chunk_rows >= n_ids) return 0;
  const uint64_t grid = (nq + tile - 1) / tile * chunks;
  return grid > 0x7fffffffull ? 0 : static_cast<uint32_t>(grid);
}

// ---- the MFMA scans (flat_mfma_scan.h): exact range search, exact filtered k-NN, histogram selection ----
constexpr uint32_t kMfmaScanQueries = 128;  // queries per workgroup: 4 waves x 32
constexpr uint32_t kMfmaScanKS = 64;        // columns per slab
constexpr uint32_t kMfmaScanTT = 4;         // 32-row tiles per super-tile
constexpr uint32_t kMfmaScanTileRows = 32 * kMfmaScanTT;

// columns the contraction accumulates over: the stride rounded up to whole slabs
inline uint32_t mfma_scan_width(uint32_t stride) { return (stride + kMfmaScanKS - 1) / kMfmaScanKS * kMfmaScanKS; }

// queries rounded up to whole query groups (constexpr: the kernels use it too)
constexpr uint64_t mfma_scan_queries_up(uint64_t nq) { return (nq + kMfmaScanQueries - 1) / kMfmaScanQueries * kMfmaScanQueries; }

struct MfmaScanChunks {
  uint64_t rows;  // rows per chunk, a multiple of kMfmaScanTileRows and at least min_rows
  uint64_t sub;   // queries per scan launch, a multiple of kMfmaScanQueries
};

// Chunks of the n > 0 rows and the split of `all` queries (a multiple of kMfmaScanQueries) over launches.  Rows
// per chunk: no more chunks than fill the CUs twice over for the query groups in flight, no fewer rows than
// min_rows.  pair_bytes(rows): what a (chunk, query) pair keeps at that chunk length, non-decreasing in rows.  All
// the queries in one launch where that fits `budget`, else half as many, down to one query group -- whose chunks
// are then as few as fit (the budget holds one group of one chunk at any length).
template <class PairBytes>
MfmaScanChunks mfma_scan_chunks(uint64_t n, uint64_t all, uint32_t cus, uint64_t min_rows, uint64_t budget,
                                PairBytes pair_bytes) {
  const uint64_t tiles = (n + kMfmaScanTileRows - 1) / kMfmaScanTileRows;
  const auto rows_for = [&](uint64_t groups, uint64_t most) {
    const uint64_t max_chunks = std::max<uint64_t>(1, std::min<uint64_t>(most, 2ull * cus / groups));
    return std::max<uint64_t>(min_rows, kMfmaScanTileRows * ((tiles + max_chunks - 1) / max_chunks));
  };
  uint64_t sub = all, rows = 0;
  for (;;) {
    rows = rows_for(sub / kMfmaScanQueries, tiles);
    const uint64_t chunks = (n + rows - 1) / rows;
    if (chunks * sub * pair_bytes(rows) <= budget) break;
    if (sub == kMfmaScanQueries) {
      rows = rows_for(1, std::max<uint64_t>(1, budget / (sub * pair_bytes(~0ull))));
      break;
    }
    sub = std::max<uint64_t>(kMfmaScanQueries, sub / 2 / kMfmaScanQueries * kMfmaScanQueries);
  }
  return {rows, sub};
}

// The grid of an MFMA scan launch, or 0 for a launch that must not run: there are queries and rows, the chunks
// are whole super-tiles and cover n exactly (the last one is not empty), rows are whole float4s, the padded
// queries are as wide as the stride rounded up to slabs, and the grid is below 2^31.
inline uint32_t mfma_scan_grid(uint64_t nq, uint64_t n, uint64_t chunk_rows, uint64_t chunks, uint32_t dim, uint32_t stride,
                               uint32_t qwidth) {
  if (nq == 0 || n == 0 || chunks == 0 || chunk_rows == 0 || chunk_rows % kMfmaScanTileRows != 0) return 0;
  if (chunks * chunk_rows < n || (chunks - 1) * chunk_rows >= n) return 0;
  if (stride < 4 || stride % 4 != 0 || qwidth != mfma_scan_width(stride) || dim > stride) return 0;
  const uint64_t grid = 8 * ((nq + kMfmaScanQueries - 1) / kMfmaScanQueries) * ((chunks + 7) / 8);
  return grid > 0x7fffffffull ? 0 : static_cast<uint32_t>(grid);
}

}  // namespace alaya_amd
