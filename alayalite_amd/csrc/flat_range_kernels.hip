// Exact range search: every eligible row with d <= radius, by the exact filtered scan's distance loop.
//
// The rows are those of an ascending id list (launch_flat_filtered_compact of flat_filtered_kernels.hip:
// mask AND validity AND below n).  Every distance is computed in f32 in the reference's summation order
// from the start (l2_sqr_avx2 / ip_sqr_avx2, restated below as in flat_filtered_kernels.hip), so the bits
// are those of flat_filtered_scan_kernel, launch_row_distances and the oracle.
//
//   1. scan    grid = row chunks (ranges of the id list) x query tiles.  A workgroup holds its tile's
//              queries in LDS (nothing else); wave w owns queries 4w..4w+3 of the tile and streams the
//              chunk's rows 32 per pass: lane group g (8 lanes) takes rows 4g..4g+3 of the pass, lane m of
//              the group the reference's accumulators 4m..4m+3.  After a pass the wave tests d <= radius
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

namespace alaya_amd {

namespace {

constexpr uint32_t kEmptyId = 0xffffffffu;
constexpr int kGatherBlock = 256;

// ---- the reference order, restated ---------------------------------------------------------------
// l2_sqr_avx2 / ip_sqr_avx2: four 8-wide accumulators over 32-element blocks (lane m of 8 owns elements
// 4m..4m+3 of each block, one fmaf per element), then the whole 8-element blocks into the first
// accumulator (lanes 0-1), the horizontal sum (xor 2, xor 4, xor 1, then (s0 + s1) + (s2 + s3)), the
// scalar tail through fmaf, and for inner products the negation last.
// Lane xor inside a group of 8 by DPP: xor 1 / 2 quad_perm, xor 4 row_ror:12 / row_ror:4 by lane bit 2.
template <int kXor>
__device__ __forceinline__ float fr_xor(float v) {
  const int x = __float_as_int(v);
  if constexpr (kXor == 1) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false));
  } else if constexpr (kXor == 2) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false));
  } else {
    const int up = __builtin_amdgcn_update_dpp(0, x, 0x12C, 0xF, 0xF, false);
    const int down = __builtin_amdgcn_update_dpp(0, x, 0x124, 0xF, 0xF, false);
    return __int_as_float((__lane_id() & 4) ? down : up);
  }
}

constexpr int kRows = 4;     // rows of a lane group per pass
constexpr int kQueries = 4;  // queries of a wave

// one 16-byte slice of each of the lane's rows against the same slice of each of the wave's queries
template <bool kIp>
__device__ __forceinline__ void fr_block(float (&acc)[kRows][kQueries][4], const float4 (&y)[kRows], const float *q,
                                         uint32_t stride, uint32_t off) {
#pragma unroll
  for (int c = 0; c < kQueries; ++c) {
    const float4 x = *reinterpret_cast<const float4 *>(q + c * stride + off);
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if constexpr (kIp) {
        acc[j][c][0] = fmaf(x.x, y[j].x, acc[j][c][0]);
        acc[j][c][1] = fmaf(x.y, y[j].y, acc[j][c][1]);
        acc[j][c][2] = fmaf(x.z, y[j].z, acc[j][c][2]);
        acc[j][c][3] = fmaf(x.w, y[j].w, acc[j][c][3]);
      } else {
        const float d0 = x.x - y[j].x, d1 = x.y - y[j].y, d2 = x.z - y[j].z, d3 = x.w - y[j].w;
        acc[j][c][0] = fmaf(d0, d0, acc[j][c][0]);
        acc[j][c][1] = fmaf(d1, d1, acc[j][c][1]);
        acc[j][c][2] = fmaf(d2, d2, acc[j][c][2]);
        acc[j][c][3] = fmaf(d3, d3, acc[j][c][3]);
      }
    }
  }
}

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
  for (uint32_t i = threadIdx.x; i < tile * stride; i += blockDim.x) {
    const uint32_t ql = i / stride, e = i - ql * stride;
    float v = 0.f;
    if (q0 + ql < p.nq && e < p.dim) {
      const uint64_t src = p.q_list ? p.q_list[p.q_first + q0 + ql] : p.q_first + q0 + ql;
      v = p.queries[src * p.q_stride + e];
    }
    qs[i] = v;
  }
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
    const uint64_t src = !live ? 0 : (p.q_list ? p.q_list[p.q_first + qi] : p.q_first + qi);
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
  for (uint64_t pb = r0; pb < r1; pb += kFlatRangePassRows) {
    // the lane group's rows, in ascending id order; a slot past the chunk recomputes the chunk's first row
    uint32_t rid[kRows];
    bool ok[kRows];
    const float *row[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const uint64_t at = pb + g * kRows + j;
      ok[j] = at < r1;
      rid[j] = p.ids[ok[j] ? at : r0];
      row[j] = p.base + static_cast<uint64_t>(rid[j]) * stride;
    }
    float acc[kRows][kQueries][4];
#pragma unroll
    for (int j = 0; j < kRows; ++j)
#pragma unroll
      for (int c = 0; c < kQueries; ++c)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[j][c][a] = 0.f;
    if (T > 0) {
      float4 y[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) y[j] = *reinterpret_cast<const float4 *>(row[j] + 4 * m);
      for (uint32_t t = 0; t < T; ++t) {
        // the next block's slices are requested before this block's arithmetic
        float4 yn[kRows];
        const uint32_t tn = t + 1 < T ? t + 1 : t;
#pragma unroll
        for (int j = 0; j < kRows; ++j) yn[j] = *reinterpret_cast<const float4 *>(row[j] + 32 * tn + 4 * m);
        fr_block<kIp>(acc, y, q, stride, 32 * t + 4 * m);
#pragma unroll
        for (int j = 0; j < kRows; ++j) y[j] = yn[j];
      }
    }
    if (m < 2) {
      for (uint32_t bb = 0; bb < nb8; ++bb) {
        const uint32_t off = 32 * T + 8 * bb + 4 * m;
        float4 y[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) y[j] = *reinterpret_cast<const float4 *>(row[j] + off);
        fr_block<kIp>(acc, y, q, stride, off);
      }
    }
    float dist[kRows][kQueries];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
#pragma unroll
      for (int c = 0; c < kQueries; ++c) {
        float a0 = acc[j][c][0], a1 = acc[j][c][1], a2 = acc[j][c][2], a3 = acc[j][c][3];
        a0 += fr_xor<2>(a0); a1 += fr_xor<2>(a1); a2 += fr_xor<2>(a2); a3 += fr_xor<2>(a3);
        a0 += fr_xor<4>(a0); a1 += fr_xor<4>(a1); a2 += fr_xor<4>(a2); a3 += fr_xor<4>(a3);
        const float s0 = a0 + fr_xor<1>(a0), s1 = a1 + fr_xor<1>(a1);
        const float s2 = a2 + fr_xor<1>(a2), s3 = a3 + fr_xor<1>(a3);
        float res = (s0 + s1) + (s2 + s3);
        for (uint32_t e = tail0; e < p.dim; ++e) {
          if constexpr (kIp) {
            res = fmaf(q[c * stride + e], row[j][e], res);
          } else {
            const float d = q[c * stride + e] - row[j][e];
            res = fmaf(d, d, res);
          }
        }
        dist[j][c] = kIp ? -res : res;
      }
    }
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
    const uint64_t dst = p.q_list ? p.q_list[p.q_first + qi] : p.q_first + qi;
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
  // Query tile, as the exact filtered scan's: 16 (four waves share each row read), smaller for a handful of
  // queries, and smaller where two workgroups would no longer fit a CU's LDS.
  uint32_t tile = nq <= 4 ? 4 : (nq <= 8 ? 8 : kFlatRangeMaxTile);
  while (tile > kFlatRangeWaveQueries && flat_range_lds(tile, stride) > kFlatRangeLdsMax / 2) tile /= 2;
  if (flat_range_lds(tile, stride) > kFlatRangeLdsMax) return r;  // tile = 0: does not fit
  r.tile = tile;
  const uint64_t q_tiles = std::max<uint64_t>(1, (nq + tile - 1) / tile);
  // no more chunks than fill the CUs twice over at this tile, rounded down
  const uint64_t max_chunks = std::max<uint64_t>(1, 2ull * cus / q_tiles);
  const uint64_t passes = (n_eligible + kFlatRangePassRows - 1) / kFlatRangePassRows;
  uint64_t chunk_rows = kFlatRangePassRows * std::max<uint64_t>(1, (passes + max_chunks - 1) / max_chunks);
  if (forced_rows) chunk_rows = (forced_rows + kFlatRangePassRows - 1) / kFlatRangePassRows * kFlatRangePassRows;
  // Staging of one (chunk, query) pair: its list and its count.  A list is never longer than the chunk.
  const auto pair_bytes = [&](uint64_t rows) { return std::min<uint64_t>(cap, rows) * 8 + 4; };
  // the cap holds at least one tile of one chunk at the longest list
  const uint64_t staging = std::max<uint64_t>(forced_staging ? forced_staging : kFlatRangeStagingCap,
                                              static_cast<uint64_t>(tile) * (static_cast<uint64_t>(cap) * 8 + 4));
  // one query tile's lists stay under the cap: where they would not, fewer and longer chunks, sized for
  // the longest list
  if ((n_eligible + chunk_rows - 1) / chunk_rows * tile * pair_bytes(chunk_rows) > staging) {
    const uint64_t cap_chunks = staging / (tile * (static_cast<uint64_t>(cap) * 8 + 4));  // >= 1
    chunk_rows = std::max(chunk_rows, kFlatRangePassRows * ((passes + cap_chunks - 1) / cap_chunks));
  }
  r.chunk_rows = chunk_rows;
  r.chunks = (n_eligible + chunk_rows - 1) / chunk_rows;
  r.slots = std::min<uint64_t>(cap, chunk_rows);
  const uint64_t all = (std::max<uint64_t>(nq, 1) + tile - 1) / tile * tile;
  r.sub_queries = all;
  if (r.chunks) {
    const uint64_t fit = staging / (r.chunks * pair_bytes(chunk_rows)) / tile * tile;  // >= tile by the above
    r.sub_queries = std::min(all, fit);
  }
  r.staging_bytes = r.chunks * std::min<uint64_t>(nq, r.sub_queries) * pair_bytes(chunk_rows);
  return r;
}

namespace {
template <bool kIp>
hipError_t scan_launch(const FlatRangeParams &p, uint32_t grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL(flat_range_scan_kernel<kIp>, dim3(grid), dim3(p.tile / kFlatRangeWaveQueries * 64), lds, s, p);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_flat_range_scan(const FlatRangeParams &p, hipStream_t s) {
  if (p.tile != 4 && p.tile != 8 && p.tile != 16) return hipErrorInvalidValue;
  if (p.cap == 0 || p.cap > kFlatRangeMaxCap || p.slots == 0 || p.slots > p.cap) return hipErrorInvalidValue;
  if (p.nq == 0 || p.chunks == 0 || p.chunk_rows == 0) return hipErrorInvalidValue;
  if (p.chunks * p.chunk_rows < p.n_ids || (p.chunks - 1) * p.chunk_rows >= p.n_ids) return hipErrorInvalidValue;
  const size_t lds = flat_range_lds(p.tile, p.stride);
  if (lds > kFlatRangeLdsMax) return hipErrorInvalidValue;
  const uint64_t grid = (p.nq + p.tile - 1) / p.tile * p.chunks;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  return p.ip ? scan_launch<true>(p, static_cast<uint32_t>(grid), lds, s)
              : scan_launch<false>(p, static_cast<uint32_t>(grid), lds, s);
}

hipError_t launch_flat_range_gather(const FlatRangeParams &p, hipStream_t s) {
  if (p.cap == 0 || p.cap > kFlatRangeMaxCap || p.nq == 0) return hipErrorInvalidValue;
  if (p.chunks && (p.slots == 0 || p.slots > p.cap)) return hipErrorInvalidValue;
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(p.nq, 1u << 16));
  hipLaunchKernelGGL(flat_range_gather_kernel, dim3(grid), dim3(kGatherBlock), 0, s, p);
  return hipGetLastError();
}

}  // namespace alaya_amd
