// What the two exact row scans share on the host: the exact filtered k-NN (flat_filtered_kernels.hip) and the
// exact range search (flat_range_kernels.hip) run the same distance pass (exact_scan_device.h) over the same
// grid -- row chunks (ranges of an ascending id list) x query tiles -- so the shape constants, the tile
// choice, the chunk sizing, the split of a batch over launches and the launch checks are written once here.
// What a scan keeps per (chunk, query) pair, and the cap on it, stays with that scan.
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

}  // namespace alaya_amd
