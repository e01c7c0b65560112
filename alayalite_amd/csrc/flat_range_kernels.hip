// Exact range search: every eligible row with d <= radius, by the exact row scans' distance pass.
//
// The rows are those of an ascending id list (launch_flat_filtered_compact of flat_filtered_kernels.hip:
// mask AND validity AND below n).  Every distance is computed in f32 in the reference's summation order
// from the start (l2_sqr_avx2 / ip_sqr_avx2, restated in exact_scan_device.h), so the bits are those of
// flat_filtered_scan_kernel, launch_row_distances and the oracle.
//
//   1. scan    grid = row chunks (ranges of the id list) x query tiles; the distance pass is
//              exact_scan_device.h's, shared with the exact filtered scan.  A workgroup's LDS holds its
//              tile's queries and nothing else.  After a pass the wave tests d <= radius
//              per (query, row) and appends the hits in id-list order -- a ballot per row slot and a prefix
//              count over the lower lane groups -- to the (chunk, query) partial list with plain vector
//              stores.  One wave owns a (chunk, query) pair, so its hit count is a register: no atomics,
//              no arrival order.  The count is not capped; the list keeps the pair's first `slots` hits.
//   2. gather  one workgroup per query sums the chunk counts and copies the chunk lists, in chunk order,
//              into the query's output row until it is full, then fills the rest with empty slots
//              (all-ones id, FLT_MAX).  range_sort_kernel then orders the row by (distance, id).
//
// The result is a function of the inputs alone: chunk order is id order, whatever the chunking, the grid,
// the tile or the split of a batch over launches.  No workgroup waits for another.
#include "flat_range_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "exact_scan_device.h"

namespace alaya_amd {

using namespace exact_scan;

namespace {

constexpr uint32_t kEmptyId = 0xffffffffu;
constexpr int kGatherBlock = 256;

}  // namespace

// Two waves per SIMD, stated: the tile's queries in LDS admit two workgroups per CU at any row width the plan
// prefers, so a third wave's registers buy nothing -- and left to aim for three (168 VGPRs) the compiler funnels
// the next block's four row loads through one register quad, each waited for before the next is issued.
template <bool kIp>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
flat_range_scan_kernel(FlatRangeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tile = p.tile, stride = p.stride;
  float *qs = reinterpret_cast<float *>(smem);  // tile x stride, zero padded
  const uint64_t q_tiles = (p.nq + tile - 1) / tile;
  const uint64_t chunk = blockIdx.x / q_tiles;
  const uint64_t q0 = (blockIdx.x % q_tiles) * tile;  // first query (of the launch) of this tile
  load_query_tile(qs, tile, stride, p.dim, p.queries, p.q_stride, p.q_list, p.q_first, q0, p.nq);
  __syncthreads();
  const int lane = __lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t g = lane >> 3, m = lane & 7;
  if (q0 + kQueries * wave >= p.nq) return;  // (no barrier below)
  const float *q = qs + static_cast<size_t>(kQueries) * wave * stride;
  // the wave's radii, hit counts and partial lists; a query slot past the launch takes no hits
  float rad[kQueries];
  uint32_t cnt[kQueries];
  uint64_t part[kQueries];
#pragma unroll
  for (int c = 0; c < kQueries; ++c) {
    const uint64_t qi = q0 + kQueries * wave + c;
    const bool live = qi < p.nq;
    const uint64_t src = !live ? 0 : query_row(p.q_list, p.q_first, qi);
    rad[c] = live ? p.radii[src] : -INFINITY;
    cnt[c] = 0;
    part[c] = (chunk * p.nq + (live ? qi : 0)) * p.slots;
  }
  const uint64_t lower = (1ull << lane) - 1ull;  // the lanes of the lower lane groups, for lane 0 of a group
  const uint64_t r0 = chunk * p.chunk_rows;
  const uint64_t r1 = r0 + p.chunk_rows < p.n_ids ? r0 + p.chunk_rows : p.n_ids;  // r0 < r1: chunks cover n_ids
  const uint32_t T = p.dim >> 5;
  const uint32_t nb8 = (p.dim - 32 * T) >> 3;
  const uint32_t tail0 = 32 * T + 8 * nb8;
  for (uint64_t pb = r0; pb < r1; pb += kScanPassRows) {
    uint32_t rid[kRows];
    bool ok[kRows];
    float dist[kRows][kQueries];
    pass<kIp>(p.ids, p.base, pb, r0, r1, q, p.dim, stride, T, nb8, tail0, g, m, dist, rid, ok);
    // Every lane of a group holds its rows' 16 distances; lane 0 of the group stands for them.  The pass's
    // rows in id-list order are (g, j) by g then j: a hit's place is the wave's count so far, plus the hits
    // of the lower groups, plus the group's own earlier hits.
#pragma unroll
    for (int c = 0; c < kQueries; ++c) {
      bool hit[kRows];
      uint64_t b[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        hit[j] = m == 0 && ok[j] && dist[j][c] <= rad[c];  // inclusive; a NaN radius or distance is no hit
        b[j] = __ballot(hit[j]);
      }
      if ((b[0] | b[1] | b[2] | b[3]) == 0ull) continue;
      uint32_t at = cnt[c];
      uint32_t all = 0;
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        at += __popcll(b[j] & lower);
        all += __popcll(b[j]);
      }
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (hit[j]) {
          if (at < p.slots) {  // inside the pair's list: slots entries from part[c]
            p.part_i[part[c] + at] = rid[j];
            p.part_d[part[c] + at] = dist[j][c];
          }
          ++at;
        }
      }
      cnt[c] += all;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kQueries; ++c) {
      const uint64_t qi = q0 + kQueries * wave + c;
      if (qi < p.nq) p.part_n[chunk * p.nq + qi] = cnt[c];
    }
  }
}

// One workgroup per query: the chunk counts summed into the query's count, the chunk lists copied in chunk
// order into the query's row until it holds `cap`, the rest of the row filled with empty slots.
__global__ void __launch_bounds__(kGatherBlock) flat_range_gather_kernel(FlatRangeParams p) {
  __shared__ uint32_t cn[kGatherBlock];
  for (uint64_t qi = blockIdx.x; qi < p.nq; qi += gridDim.x) {
    const uint64_t dst = query_row(p.q_list, p.q_first, qi);
    const uint64_t out = dst * p.cap;
    uint32_t total = 0, off = 0;
    for (uint64_t c0 = 0; c0 < p.chunks; c0 += kGatherBlock) {
      __syncthreads();
      if (c0 + threadIdx.x < p.chunks) cn[threadIdx.x] = p.part_n[(c0 + threadIdx.x) * p.nq + qi];
      __syncthreads();
      const uint32_t here = p.chunks - c0 < kGatherBlock ? static_cast<uint32_t>(p.chunks - c0) : kGatherBlock;
      for (uint32_t cc = 0; cc < here; ++cc) {
        const uint32_t n_c = cn[cc];
        total += n_c;
        const uint32_t take = min(min(n_c, p.slots), p.cap - off);  // off <= cap
        const uint64_t src = ((c0 + cc) * p.nq + qi) * p.slots;
        for (uint32_t e = threadIdx.x; e < take; e += kGatherBlock) {
          p.out_ids[out + off + e] = p.part_i[src + e];
          p.out_dists[out + off + e] = p.part_d[src + e];
        }
        off += take;
      }
    }
    for (uint32_t e = off + threadIdx.x; e < p.cap; e += kGatherBlock) {
      p.out_ids[out + e] = kEmptyId;
      p.out_dists[out + e] = FLT_MAX;
    }
    if (threadIdx.x == 0) p.out_counts[dst] = total;
  }
}

// ---- host side -------------------------------------------------------------------------------------
size_t flat_range_lds(uint32_t tile, uint32_t stride) { return static_cast<size_t>(tile) * stride * 4; }

FlatRangePlan flat_range_plan(uint64_t n_eligible, uint64_t nq, uint32_t cap, uint32_t stride, uint32_t cus,
                              uint64_t forced_rows, uint64_t forced_staging) {
  FlatRangePlan r{};
  cap = std::min<uint32_t>(std::max<uint32_t>(cap, 1), kFlatRangeMaxCap);
  cus = std::max<uint32_t>(cus, 1);
  const uint32_t tile = scan_tile(nq, [&](uint32_t t) { return flat_range_lds(t, stride); });
  if (tile == 0) return r;  // does not fit
  r.tile = tile;
  uint64_t chunk_rows = scan_chunk_rows(n_eligible, nq, tile, cus, forced_rows);
  // Staging of one (chunk, query) pair: its list and its count.  A list is never longer than the chunk.
  const auto pair_bytes = [&](uint64_t rows) { return std::min<uint64_t>(cap, rows) * 8 + 4; };
  // the cap holds at least one tile of one chunk at the longest list
  const uint64_t staging = std::max<uint64_t>(forced_staging ? forced_staging : kFlatRangeStagingCap,
                                              static_cast<uint64_t>(tile) * (static_cast<uint64_t>(cap) * 8 + 4));
  // one query tile's lists stay under the cap: where they would not, fewer and longer chunks, sized for
  // the longest list
  if ((n_eligible + chunk_rows - 1) / chunk_rows * tile * pair_bytes(chunk_rows) > staging) {
    const uint64_t cap_chunks = staging / (tile * (static_cast<uint64_t>(cap) * 8 + 4));  // >= 1
    chunk_rows = std::max(chunk_rows, kScanPassRows * ((scan_passes(n_eligible) + cap_chunks - 1) / cap_chunks));
  }
  r.chunk_rows = chunk_rows;
  r.chunks = (n_eligible + chunk_rows - 1) / chunk_rows;
  r.slots = std::min<uint64_t>(cap, chunk_rows);
  r.sub_queries = scan_sub_queries(nq, tile, r.chunks, staging, pair_bytes(chunk_rows));  // >= tile by the above
  r.staging_bytes = r.chunks * std::min<uint64_t>(nq, r.sub_queries) * pair_bytes(chunk_rows);
  return r;
}

namespace {
template <bool kIp>
hipError_t scan_launch(const FlatRangeParams &p, uint32_t grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL(flat_range_scan_kernel<kIp>, dim3(grid), dim3(p.tile / kScanWaveQueries * 64), lds, s, p);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_flat_range_scan(const FlatRangeParams &p, hipStream_t s) {
  const uint32_t grid = scan_grid(p.tile, p.nq, p.n_ids, p.chunk_rows, p.chunks);
  if (grid == 0 || p.cap == 0 || p.cap > kFlatRangeMaxCap || p.slots == 0 || p.slots > p.cap) return hipErrorInvalidValue;
  const size_t lds = flat_range_lds(p.tile, p.stride);
  if (lds > kScanLdsMax) return hipErrorInvalidValue;
  return p.ip ? scan_launch<true>(p, grid, lds, s) : scan_launch<false>(p, grid, lds, s);
}

hipError_t launch_flat_range_gather(const FlatRangeParams &p, hipStream_t s) {
  if (p.cap == 0 || p.cap > kFlatRangeMaxCap || p.nq == 0) return hipErrorInvalidValue;
  if (p.chunks && (p.slots == 0 || p.slots > p.cap)) return hipErrorInvalidValue;
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(p.nq, 1u << 16));
  hipLaunchKernelGGL(flat_range_gather_kernel, dim3(grid), dim3(kGatherBlock), 0, s, p);
  return hipGetLastError();
}

}  // namespace alaya_amd
