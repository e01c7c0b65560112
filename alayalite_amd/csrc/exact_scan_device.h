// The distance pass of the two exact row scans: flat_filtered_scan_kernel (exact filtered k-NN) and
// flat_range_scan_kernel (exact range search) compute their distances here and differ only in what they do
// with a distance once it is known.
//
// A workgroup holds its tile's queries in LDS (load_query_tile); wave w owns queries 4w..4w+3 of the tile and
// streams a chunk of an ascending id list 32 rows per pass: lane group g (8 lanes) takes rows 4g..4g+3 of the
// pass, lane m of the group the reference's accumulators 4m..4m+3.  A lane's 16-byte slice of each of its 4 rows
// meets the 4 queries' slices before it is dropped: 64 accumulators, 4 global and 4 LDS 16-byte reads per 64
// fmaf.  The waves of a workgroup read the same rows at the same time, so a row leaves memory once per tile.
//
// The reference order, restated (l2_sqr_avx2 / ip_sqr_avx2): four 8-wide accumulators over 32-element blocks
// (lane m of 8 owns elements 4m..4m+3 of each block, one fmaf per element), then the whole 8-element blocks
// into the first accumulator (lanes 0-1), the horizontal sum (xor 2, xor 4, xor 1, then (s0 + s1) + (s2 + s3)),
// the scalar tail through fmaf, and for inner products the negation last.  Every distance is f32 in that order
// from the start, so the bits are those of launch_row_distances, flat_kernels.hip's exact_l2 / exact_ip and the
// oracle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exact_scan_plan.h"

namespace alaya_amd {
namespace exact_scan {

constexpr int kRows = 4;     // rows of a lane group per pass
constexpr int kQueries = 4;  // queries of a wave
static_assert(uint32_t(kQueries) == kScanWaveQueries && uint32_t(8 * kRows) == kScanPassRows,
              "the pass is 8 lane groups x 4 rows x 4 queries");

// Query qi of a launch is row q_list[q_first + qi] of the caller's queries and outputs; q_list null = row q_first + qi.
__device__ __forceinline__ uint64_t query_row(const uint32_t *q_list, uint64_t q_first, uint64_t qi) {
  return q_list ? q_list[q_first + qi] : q_first + qi;
}

// The workgroup's query tile (queries q0 .. q0 + tile of the launch's nq) into qs: tile x stride, zero padded
// past dim and past the launch's last query.  The caller synchronises.
__device__ __forceinline__ void load_query_tile(float *qs, uint32_t tile, uint32_t stride, uint32_t dim,
                                                const float *queries, uint32_t q_stride, const uint32_t *q_list,
                                                uint64_t q_first, uint64_t q0, uint64_t nq) {
  for (uint32_t i = threadIdx.x; i < tile * stride; i += blockDim.x) {
    const uint32_t ql = i / stride, e = i - ql * stride;
    float v = 0.f;
    if (q0 + ql < nq && e < dim) v = queries[query_row(q_list, q_first, q0 + ql) * q_stride + e];
    qs[i] = v;
  }
}

// Lane xor inside a group of 8 by DPP: xor 1 / 2 quad_perm, xor 4 row_ror:12 / row_ror:4 by lane bit 2.
template <int kXor>
__device__ __forceinline__ float lane_xor(float v) {
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

// one 16-byte slice of each of the lane's rows against the same slice of each of the wave's queries
template <bool kIp>
__device__ __forceinline__ void block(float (&acc)[kRows][kQueries][4], const float4 (&y)[kRows], const float *q,
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

// One pass of lane group g, lane m: entries pb + 4g .. pb + 4g + 3 of ids (the chunk is [r0, r1)) against the
// wave's 4 queries at q (LDS rows of `stride` floats).  rid / ok: the rows' ids and whether the slot is inside
// the chunk; dist[j][c]: row j against query c, in every lane of the group.  T = dim / 32 whole blocks, nb8
// whole 8-element blocks after them, tail0 the first element of the scalar tail.
template <bool kIp>
__device__ __forceinline__ void pass(const uint32_t *ids, const float *base, uint64_t pb, uint64_t r0, uint64_t r1,
                                     const float *q, uint32_t dim, uint32_t stride, uint32_t T, uint32_t nb8,
                                     uint32_t tail0, uint32_t g, uint32_t m, float (&dist)[kRows][kQueries],
                                     uint32_t (&rid)[kRows], bool (&ok)[kRows]) {
  // the lane group's rows, in ascending id order; a slot past the chunk recomputes the chunk's first row
  const float *row[kRows];
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const uint64_t at = pb + g * kRows + j;
    ok[j] = at < r1;
    rid[j] = ids[ok[j] ? at : r0];
    row[j] = base + static_cast<uint64_t>(rid[j]) * stride;
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
      block<kIp>(acc, y, q, stride, 32 * t + 4 * m);
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
      block<kIp>(acc, y, q, stride, off);
    }
  }
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
#pragma unroll
    for (int c = 0; c < kQueries; ++c) {
      float a0 = acc[j][c][0], a1 = acc[j][c][1], a2 = acc[j][c][2], a3 = acc[j][c][3];
      a0 += lane_xor<2>(a0); a1 += lane_xor<2>(a1); a2 += lane_xor<2>(a2); a3 += lane_xor<2>(a3);
      a0 += lane_xor<4>(a0); a1 += lane_xor<4>(a1); a2 += lane_xor<4>(a2); a3 += lane_xor<4>(a3);
      const float s0 = a0 + lane_xor<1>(a0), s1 = a1 + lane_xor<1>(a1);
      const float s2 = a2 + lane_xor<1>(a2), s3 = a3 + lane_xor<1>(a3);
      float res = (s0 + s1) + (s2 + s3);
      for (uint32_t e = tail0; e < dim; ++e) {
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
}

}  // namespace exact_scan
}  // namespace alaya_amd
