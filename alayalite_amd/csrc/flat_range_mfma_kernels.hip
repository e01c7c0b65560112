// Exact range search on the MFMA scan: prove most (query, row) pairs by a matrix contraction, verify the band.
//
//   1. prepare  one wave per query of the launch: the query zero padded to whole slabs, |q|^2, and the two
//               thresholds lo <= hi of flat_range_bound.h.
//   2. scan     flat_range_mfma_kernel<kIp>: the work split and the streaming pass that flat_mfma_scan.h describes,
//               with the tile's eligibility word mask AND validity AND below n.  The consumer: per accumulator
//               register of a super-tile d~, two compares, the tile's eligibility bit and a ballot: no
//               candidate bit set, next register.  Otherwise the register's two ballots go to a per-wave LDS
//               list that is settled after the super-tile's compares, per query of the register: the pairs that
//               need the exact distance -- the band bits, and every candidate bit while the query's count is
//               below `slots` -- are computed 8 at a time, a group of 8 lanes per pair in exact_scan_device.h's
//               order, and the hits appended in row order with plain vector stores; proven bits past
//               `slots` add their popcount.  One wave owns a (chunk, query) pair: counts are registers (lane q
//               of the wave holds query q's), nothing is atomic, no workgroup waits for another.
//   3. reduce   the per-wave counters (pairs verified, band pairs, pairs proven) summed by one workgroup.
//
// Resources: beside the pass's registers a lane holds 48 VGPRs of thresholds: 245 VGPRs + 64 AGPRs for L2, 221 +
// 64 for IP, no scratch, one wave per SIMD.
#include "flat_range_mfma_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "exact_scan_device.h"
#include "flat_mfma_scan.h"
#include "flat_range_bound.h"

namespace alaya_amd {

using exact_scan::query_row;
using namespace mfma_scan;

__global__ void __launch_bounds__(256) flat_range_mfma_prepare_kernel(FlatRangeMfmaParams p) {
  const uint64_t nq_up = mfma_scan_queries_up(p.nq);
  const uint64_t qi = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (qi >= nq_up) return;
  const int lane = __lane_id();
  const bool live = qi < p.nq;
  const uint64_t src = live ? query_row(p.q_list, p.q_first, qi) : 0;
  float sum = 0.f;
  for (uint32_t e = lane; e < p.qwidth; e += 64) {
    const float v = live && e < p.dim ? p.queries[src * p.q_stride + e] : 0.f;
    p.qpad[qi * p.qwidth + e] = v;
    sum = fmaf(v, v, sum);
  }
  for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x);
  if (lane == 0) {
    const float rad = live ? p.radii[src] : -INFINITY;
    FlatRangeBound b = flat_range_bound(p.ip != 0, rad, sum, p.max_norm, p.qwidth, kFlatSplit);
    if (!live) b.lo = b.hi = -INFINITY;
    p.qmeta[qi] = sum;
    p.qmeta[nq_up + qi] = b.lo;
    p.qmeta[2 * nq_up + qi] = b.hi;
    p.qmeta[3 * nq_up + qi] = rad;
  }
}

template <bool kIp>
__global__ void __launch_bounds__(256) flat_range_mfma_kernel(FlatRangeMfmaParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 tile[kTileLds];
  __shared__ uint64_t pend[4][TT * 16][2];  // per wave: the (candidate, proven) ballots of a super-tile's registers
  const int lane = __lane_id();
  const int wave = threadIdx.x >> 6;
  const int col = lane & 31, h = lane >> 5;
  const uint32_t g = lane >> 3, m = lane & 7;
  const uint64_t nq_up = mfma_scan_queries_up(p.nq);
  const uint32_t nqg = static_cast<uint32_t>(nq_up / kMfmaScanQueries);
  // XCD-aware block -> (query group, chunk): the query groups of one chunk share an XCD label
  const uint32_t b = blockIdx.x;
  const uint32_t qg = (b / 8) % nqg;
  const uint64_t chunk = (b % 8) + 8ull * (b / (8 * nqg));
  if (chunk >= p.chunks) return;
  const uint64_t r0 = chunk * p.chunk_rows;
  const uint64_t r1 = min(p.n, r0 + p.chunk_rows);  // r0 < r1: the chunks cover n
  const int nslab = static_cast<int>(p.qwidth / KS);
  const uint64_t q0 = static_cast<uint64_t>(qg) * kMfmaScanQueries + wave * 32;  // the wave's first query

  // per accumulator register: the thresholds of its query (and |q|^2 for L2)
  float lo[16], hi[16], qn[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const uint64_t qi = query_slot(q0, r, h);
    qn[r] = kIp ? 0.f : p.qmeta[qi];
    lo[r] = p.qmeta[nq_up + qi];
    hi[r] = p.qmeta[2 * nq_up + qi];
  }
  // per lane q < 32: query q0 + q's radius and hit count
  const float radv = p.qmeta[3 * nq_up + q0 + col];
  uint32_t cntv = 0;
  uint32_t st_verified = 0, st_band = 0, st_proven = 0;
  const uint64_t lower = (1ull << lane) - 1ull;

  const float4 *qrow = reinterpret_cast<const float4 *>(p.qpad + (q0 + col) * p.qwidth + h * (KS / 2));
  float4 an[KS / 8];
  auto load_a = [&](int s) {
#pragma unroll
    for (int j = 0; j < KS / 8; ++j) an[j] = qrow[s * (KS / 4) + j];
  };

  // cooperative unit load: 32 rows x KS columns, 256 threads, float4 each; rows past n read row n - 1 (their
  // eligibility bits are clear), columns past stride are zeroed when stored
  auto load_unit = [&](uint64_t row0, uint32_t c0, float4 (&reg)[kPerThread]) {
#pragma unroll
    for (int v = 0; v < kPerThread; ++v) {
      const int idx = threadIdx.x + v * 256;
      const uint64_t row = min<uint64_t>(row0 + idx / kVecPerRow, p.n - 1);
      const uint32_t c = min<uint32_t>(c0 + (idx % kVecPerRow) * 4, p.stride - 4);
      reg[v] = *reinterpret_cast<const float4 *>(p.base + row * p.stride + c);
    }
  };
  auto store_unit = [&](int buf, uint32_t c0, const float4 (&reg)[kPerThread]) {
#pragma unroll
    for (int v = 0; v < kPerThread; ++v) {
      const int idx = threadIdx.x + v * 256;
      const bool in = c0 + (idx % kVecPerRow) * 4 < p.stride;
      const float4 x = in ? reg[v] : make_float4(0.f, 0.f, 0.f, 0.f);
      __bf16 *th = tile + buf * 2 * kHalf + (idx / kVecPerRow) * kBPitch + (idx % kVecPerRow) * 4;
      bf16x4 hv, lv;
      __bf16 xh, xl;
      split_bf16(x.x, xh, xl); hv[0] = xh; lv[0] = xl;
      split_bf16(x.y, xh, xl); hv[1] = xh; lv[1] = xl;
      split_bf16(x.z, xh, xl); hv[2] = xh; lv[2] = xl;
      split_bf16(x.w, xh, xl); hv[3] = xh; lv[3] = xl;
      *reinterpret_cast<bf16x4 *>(th) = hv;
      *reinterpret_cast<bf16x4 *>(th + kHalf) = lv;
    }
  };

  // One query of an accumulator register: qs its slot in the wave, row0 the tile's first row, cand / sure the
  // tile's candidate and proven bits for it.  Wave-uniform.
  auto settle = [&](int qs, uint64_t row0, uint32_t cand, uint32_t sure) {
    const uint64_t qi = q0 + qs;
    if (cand == 0 || qi >= p.nq) return;
    uint32_t cnt = read_lane(cntv, qs);
    uint32_t need = cnt < p.slots ? cand : (cand & ~sure);
    const uint32_t proven = __popc(sure & ~need);
    st_verified += __popc(need);
    st_band += __popc(need & ~sure);
    st_proven += proven;
    cnt += proven;  // (proven > 0 only past `slots`: nothing more is stored, the order no longer matters)
    if (need != 0) {
      const float rad = read_lane_f(radv, qs);
      const float *q = p.qpad + qi * p.qwidth;
      const uint64_t part = (chunk * p.nq + qi) * p.slots;
      while (need != 0) {
        // the next 8 pairs in ascending row order, one per lane group; an idle group recomputes the first
        uint32_t mine = __builtin_ctz(need);
        bool active = false;
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
          if (need != 0) {
            const uint32_t bit = __builtin_ctz(need);
            if (g == i) {
              mine = bit;
              active = true;
            }
            need &= need - 1;
          }
        }
        const uint64_t rid = row0 + mine;  // < n: the eligibility word has no bit past n
        const float d = exact_scan::pair_distance<kIp>(q, p.base + rid * p.stride, p.dim, m);
        const bool hit = active && m == 0 && d <= rad;  // inclusive; a NaN radius or distance is no hit
        const uint64_t hb = __ballot(hit);
        if (hit) {
          const uint32_t at = cnt + __popcll(hb & lower);
          if (at < p.slots) {
            p.part_i[part + at] = static_cast<uint32_t>(rid);
            p.part_d[part + at] = d;
          }
        }
        cnt += __popcll(hb);
      }
    }
    if (lane == qs) cntv = cnt;
  };

  float4 stage[kPerThread];
  load_a(0);
  load_unit(r0, 0, stage);
  store_unit(0, 0, stage);
  __syncthreads();
  int buf = 0;
  for (uint64_t sup = r0; sup < r1; sup += kTile * TT) {
    const int ntiles = static_cast<int>(min<uint64_t>(TT, (r1 - sup + kTile - 1) / kTile));
    const bool last_sup = sup + kTile * TT >= r1;
    float bn[TT];
    uint32_t el[TT];  // the tiles' eligibility words: mask AND validity AND below n
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const uint64_t row0 = sup + kTile * t;
      bn[t] = kIp ? 0.f : p.norms[min<uint64_t>(row0 + col, p.n - 1)];
      uint32_t w = 0;
      if (row0 < r1) {
        w = p.words[row0 >> 5];
        if (p.valid != nullptr) w &= p.valid[row0 >> 5];
        if (p.n - row0 < 32) w &= (1u << (p.n - row0)) - 1u;
      }
      el[t] = w;
    }
    f32x16 c[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) c[t] = f32x16{};
    for (int s = 0; s < nslab; ++s) {
      // this slab's A fragments: k-step st of lane (col, h) holds columns s KS + h KS/2 + 8 st + j
      bf16x8 ah[KS / 16], al[KS / 16];
#pragma unroll
      for (int st = 0; st < KS / 16; ++st) {
        const float4 u = an[2 * st], w = an[2 * st + 1];
        const float v8[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          __bf16 xh, xl;
          split_bf16(v8[j], xh, xl);
          ah[st][j] = xh;
          al[st][j] = xl;
        }
      }
      if (s + 1 < nslab || !last_sup) load_a(s + 1 < nslab ? s + 1 : 0);  // the next slab's slice in flight
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        if (t < ntiles) {  // wave-uniform, and the same in every wave of the workgroup
          // the unit after (s, t): (s, t + 1), else (s + 1, 0), else the next super-tile's (0, 0)
          uint64_t nrow = 0;
          uint32_t ncol = 0;
          bool next = true;
          if (t + 1 < ntiles) {
            nrow = sup + kTile * (t + 1);
            ncol = s * KS;
          } else if (s + 1 < nslab) {
            nrow = sup;
            ncol = (s + 1) * KS;
          } else if (!last_sup) {
            nrow = sup + kTile * TT;
            ncol = 0;
          } else {
            next = false;
          }
          if (next) load_unit(nrow, ncol, stage);
          const __bf16 *tb = tile + buf * 2 * kHalf + col * kBPitch + h * (KS / 2);
#pragma unroll
          for (int st = 0; st < KS / 16; ++st) {
            const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(tb + 8 * st);
            const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(tb + kHalf + 8 * st);
            c[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[st], bh, c[t], 0, 0, 0);
            c[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[st], bl, c[t], 0, 0, 0);
            c[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[st], bh, c[t], 0, 0, 0);
          }
          if (next) {
            store_unit(buf ^ 1, ncol, stage);
            buf ^= 1;
          }
          __syncthreads();
        }
      }
    }
    // thresholds: two compares, the eligibility bit and a ballot per accumulator register; the registers with
    // a candidate bit leave their two ballots in the wave's LDS list and are settled below, in (tile, register)
    // order -- for any one query that is ascending row order
    uint64_t pending = 0;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if (t < ntiles && el[t] != 0) {
        const bool eligible = (el[t] >> col) & 1u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = approx_distance<kIp>(qn[r], bn[t], c[t][r]);
          const bool cand = eligible && !(d > hi[r]);  // NaN: the band
          const uint64_t cm = __ballot(cand);
          if (cm == 0ull) continue;
          const uint64_t sm = __ballot(eligible && d <= lo[r]);
          if (lane == 0) {
            pend[wave][t * 16 + r][0] = cm;
            pend[wave][t * 16 + r][1] = sm;
          }
          pending |= 1ull << (t * 16 + r);
        }
      }
    }
    if (pending != 0ull) {
      wave_fence();
      while (pending != 0ull) {
        const int idx = __builtin_ctzll(pending);
        pending &= pending - 1ull;
        const uint64_t cm = uniform64(pend[wave][idx][0]), sm = uniform64(pend[wave][idx][1]);
        const int t = idx >> 4, r = idx & 15;
        const int qs = query_slot(0, r, 0);
#pragma unroll 1
        for (int hh = 0; hh < 2; ++hh)
          settle(qs + 4 * hh, sup + kTile * t, static_cast<uint32_t>(cm >> (32 * hh)), static_cast<uint32_t>(sm >> (32 * hh)));
      }
      wave_fence();
    }
  }
  // the wave's counts and counters
  if (col + q0 < p.nq && h == 0) p.part_n[chunk * p.nq + q0 + col] = cntv;
  if (lane == 0) {
    uint32_t *ws = p.wave_stats + (chunk * (nq_up / 32) + q0 / 32) * 3;
    ws[0] = st_verified;
    ws[1] = st_band;
    ws[2] = st_proven;
  }
}

__global__ void __launch_bounds__(256) flat_range_mfma_reduce_kernel(const uint32_t *wave_stats, uint64_t waves,
                                                                     unsigned long long *stats) {
  reduce_wave_stats<3>(wave_stats, waves, stats);
}

__global__ void flat_range_mfma_clear_kernel(unsigned long long *stats) { clear_stats<3>(stats); }

// ---- host side -------------------------------------------------------------------------------------
FlatRangeMfmaPlan flat_range_mfma_plan(uint64_t n, uint64_t nq, uint32_t cap, uint32_t cus) {
  FlatRangeMfmaPlan r{};
  cap = std::min<uint32_t>(std::max<uint32_t>(cap, 1), kFlatRangeMaxCap);
  cus = std::max<uint32_t>(cus, 1);
  const uint64_t all = mfma_scan_queries_up(std::max<uint64_t>(nq, 1));
  r.sub_queries = all;
  if (n == 0) return r;
  // a chunk is no shorter than twice its list: of a chunk full of hits at least half are counted without a distance
  const uint64_t min_rows = (2ull * cap + kMfmaScanTileRows - 1) / kMfmaScanTileRows * kMfmaScanTileRows;
  const auto pair_bytes = [&](uint64_t rows) { return std::min<uint64_t>(cap, rows) * 8 + 4; };
  const MfmaScanChunks c = mfma_scan_chunks(n, all, cus, min_rows, kFlatRangeStagingCap, pair_bytes);
  r.chunk_rows = c.rows;
  r.chunks = (n + c.rows - 1) / c.rows;
  r.sub_queries = c.sub;
  r.slots = std::min<uint64_t>(cap, c.rows);
  r.staging_bytes = r.chunks * std::min(all, c.sub) * pair_bytes(c.rows);
  return r;
}

hipError_t launch_flat_range_mfma_prepare(const FlatRangeMfmaParams &p, hipStream_t s) {
  if (p.nq == 0 || p.qwidth == 0 || p.qwidth % kMfmaScanKS != 0 || p.qwidth < p.dim) return hipErrorInvalidValue;
  const uint64_t nq_up = mfma_scan_queries_up(p.nq);
  hipLaunchKernelGGL(flat_range_mfma_prepare_kernel, dim3(static_cast<uint32_t>(nq_up / 4)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_flat_range_mfma_scan(const FlatRangeMfmaParams &p, hipStream_t s) {
  const uint32_t grid = mfma_scan_grid(p.nq, p.n, p.chunk_rows, p.chunks, p.dim, p.stride, p.qwidth);
  if (grid == 0) return hipErrorInvalidValue;
  if (p.cap == 0 || p.cap > kFlatRangeMaxCap || p.slots == 0 || p.slots > p.cap) return hipErrorInvalidValue;
  if (p.ip)
    hipLaunchKernelGGL(flat_range_mfma_kernel<true>, dim3(grid), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(flat_range_mfma_kernel<false>, dim3(grid), dim3(256), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flat_range_mfma_reduce_kernel, dim3(1), dim3(256), 0, s, p.wave_stats,
                     p.chunks * (mfma_scan_queries_up(p.nq) / 32), p.stats);
  return hipGetLastError();
}

hipError_t launch_flat_range_mfma_clear(unsigned long long *stats, hipStream_t s) {
  hipLaunchKernelGGL(flat_range_mfma_clear_kernel, dim3(1), dim3(64), 0, s, stats);
  return hipGetLastError();
}

}  // namespace alaya_amd
