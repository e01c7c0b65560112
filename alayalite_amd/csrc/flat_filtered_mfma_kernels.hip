// Exact filtered k-NN on the MFMA scan: a top-k search is a range search whose radius shrinks.
//
//   1. prepare  one wave per query of the launch: the query zero padded to whole slabs and |q|^2; the first
//               threshold is +inf (-inf for the padding queries past nq, which then never have a candidate).
//   2. scan     flat_filtered_mfma_kernel<kIp>: the work split and the streaming pass that flat_mfma_scan.h
//               describes, with the tile's eligibility word mask AND validity AND below n.
//
//               The consumer.  One wave owns a (chunk, query) pair and its list of up to k entries, which
//               lives in the partial buffers in global memory (32 queries x 224 x 8 bytes per wave do not fit
//               the LDS): ascending by (distance, id), `cnt` entries long.  Lane q < 32 of the wave holds query
//               q's count and worst entry (w, id), FLT_MAX and the all-ones id while the list is not full, and a
//               per-wave LDS array holds its threshold t: +inf until the list is full, then
//               flat_range_bound(w).hi.  After a super-tile's last slab the wave goes through its tiles one at a
//               time: per accumulator register one compare against the register's copy of t, the tile's
//               eligibility bit and a ballot; an eligible pair is a candidate when !(d~ > t), so NaN pairs are.
//               The registers with a candidate leave their ballot in a per-wave LDS list and are settled in
//               ascending row order: 8 pairs at a time get the reference-order distance (a group of 8 lanes per
//               pair, exact_scan::pair_distance), and the ones before the worst entry under ff_before's rule are
//               inserted one after another -- every lane reads up to 4 entries, a ballot counts the ones
//               before the newcomer, the rest move up by one.  A NaN distance is before nothing, as in the f32
//               scan.  When a full list changed, w is its last entry and t is recomputed on the device; the
//               registers' copies are refreshed from the LDS array after the tile, before the next tile's
//               compares.  Exact because rows arrive in ascending id: a later row replaces the worst entry only
//               if d_ref < w, and d~ > hi(w) proves d_ref > w; thresholds only shrink, so a stale copy only
//               verifies more.  Only one wave writes a list, nothing is atomic, no workgroup waits for another.
//               A lane reads entries that another lane of its wave wrote: after an insertion's stores a
//               workgroup-scope fence waits for them (the lanes of a wave share the CU's vector cache).
//               When the chunk ends the slots past cnt are written empty: (0xffffffff, FLT_MAX).
//   3. reduce   the per-wave counters (pairs verified, pairs inserted) summed by one workgroup.
//
// Resources (the compiler's kernel-resource-usage remarks, built without the packed f32 instructions as
// flat_range_mfma_kernels.hip is): L2 256 VGPRs + 64 AGPRs, IP 232 + 64, 106 SGPRs each, no scratch, 19,456
// bytes of LDS per workgroup, one wave per SIMD -- as the range kernel.  The L2 kernel is at the VGPR limit: the
// 16 lower thresholds the range kernel keeps are gone, the list's 8 entry registers and the bound's arithmetic
// take their place.
#include "flat_filtered_mfma_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "exact_scan_device.h"
#include "flat_mfma_scan.h"
#include "flat_range_bound.h"

namespace alaya_amd {

using exact_scan::query_row;
using namespace mfma_scan;

namespace {

constexpr uint32_t kEmptyId = 0xffffffffu;

// the list's stores done before any lane of the wave reads the list again
__device__ __forceinline__ void list_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// flat_filtered_kernels.hip's order of every selection: smaller distance first, then smaller id
__device__ __forceinline__ bool ff_before(float da, uint32_t ia, float db, uint32_t ib) {
  return (da < db) | ((da == db) & (ia < ib));
}

}  // namespace

__global__ void __launch_bounds__(256) flat_filtered_mfma_prepare_kernel(FlatFilteredMfmaParams p) {
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
    p.qmeta[qi] = sum;
    p.qmeta[nq_up + qi] = live ? INFINITY : -INFINITY;
  }
}

template <bool kIp>
__global__ void __launch_bounds__(256) flat_filtered_mfma_kernel(FlatFilteredMfmaParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 tile[kTileLds];
  __shared__ uint64_t pend[4][16];  // per wave: the candidate ballots of a tile's registers
  __shared__ float thr[4][32];      // per wave: its queries' thresholds
  const int lane = __lane_id();
  const int wave = threadIdx.x >> 6;
  const int col = lane & 31, h = lane >> 5;
  const uint32_t g = lane >> 3, m = lane & 7;
  const uint32_t k = p.k;
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

  // per accumulator register: its query's threshold (and |q|^2 for L2)
  float hi[16], qn[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const uint64_t qi = query_slot(q0, r, h);
    qn[r] = kIp ? 0.f : p.qmeta[qi];
    hi[r] = p.qmeta[nq_up + qi];
  }
  if (h == 0) thr[wave][col] = p.qmeta[nq_up + q0 + col];
  // per lane q < 32: query q0 + q's entries and worst entry (the empty slot while the list is not full)
  uint32_t cntv = 0, wiv = kEmptyId;
  float wdv = FLT_MAX;
  uint32_t st_verified = 0, st_inserted = 0;
  bool dirty = false;  // a threshold of the wave changed since the registers' copies were read (wave-uniform)

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

  // (d, id), which is before the list's worst entry (wd, wi), into the sorted list of cnt entries: lane l holds
  // entries l, l + 64, ... (k <= 256); the ones not before the newcomer move up by one, and of a full list the
  // last drops out.  Leaves the new count and worst entry.  Wave-uniform.
  auto insert = [&](float *Ld, uint32_t *Li, uint32_t &cnt, float d, uint32_t id, float &wd, uint32_t &wi) {
    float ed[4];
    uint32_t ei[4];
    uint32_t pos = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t e = lane + 64 * r;
      ed[r] = FLT_MAX;
      ei[r] = kEmptyId;
      if (e < cnt) {
        ed[r] = Ld[e];
        ei[r] = Li[e];
      }
      pos += __popcll(__ballot(e < cnt && ff_before(ed[r], ei[r], d, id)));
    }
    // pos <= cnt, and pos < k: a full list's last entry is not before the newcomer
    const uint32_t after = cnt < k ? cnt + 1 : k;
    if (after == k) {  // the full list's last entry: the newcomer, or what was entry k - 2
      if (pos + 1 == k) {
        wd = d;
        wi = id;
      } else {
        const uint32_t e2 = k - 2, r2 = e2 >> 6;
        const float vd = r2 == 0 ? ed[0] : r2 == 1 ? ed[1] : r2 == 2 ? ed[2] : ed[3];
        const uint32_t vi = r2 == 0 ? ei[0] : r2 == 1 ? ei[1] : r2 == 2 ? ei[2] : ei[3];
        wd = read_lane_f(vd, e2 & 63);
        wi = read_lane(vi, e2 & 63);
      }
    }
    // every lane's loads have returned: the ballots above read them
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t e = lane + 64 * r;
      if (e >= pos && e < cnt && e + 1 < k) {
        Ld[e + 1] = ed[r];
        Li[e + 1] = ei[r];
      }
    }
    if (lane == 0 && pos < k) {  // (always: see above; the store stays inside the list whatever was read)
      Ld[pos] = d;
      Li[pos] = id;
    }
    cnt = after;
    list_fence();
  };

  // One query of an accumulator register: qs its slot in the wave, row0 the tile's first row, cand the tile's
  // candidate bits for it.  Wave-uniform.
  auto settle = [&](int qs, uint64_t row0, uint32_t cand) {
    const uint64_t qi = q0 + qs;
    if (cand == 0 || qi >= p.nq) return;
    uint32_t cnt = read_lane(cntv, qs);
    float wd = read_lane_f(wdv, qs);
    uint32_t wi = read_lane(wiv, qs);
    st_verified += __popc(cand);
    const float *q = p.qpad + qi * p.qwidth;
    const uint64_t part = (chunk * p.nq + qi) * k;
    bool changed = false;
    uint32_t need = cand;
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
      // (a NaN distance is before nothing)
      uint64_t offer = __ballot(active && m == 0 && ff_before(d, static_cast<uint32_t>(rid), wd, wi));
      while (offer != 0ull) {  // lane groups in ascending order: ascending rows
        const int src = __builtin_ctzll(offer);
        offer &= offer - 1ull;
        const float cd = read_lane_f(d, src);
        const uint32_t ci = read_lane(static_cast<uint32_t>(rid), src);
        if (!ff_before(cd, ci, wd, wi)) continue;  // the worst entry moved since the offer
        insert(p.part_d + part, p.part_i + part, cnt, cd, ci, wd, wi);
        ++st_inserted;
        changed = true;
      }
    }
    if (changed) {
      if (cnt == k) {
        const float t = flat_range_bound(kIp, wd, p.qmeta[qi], p.max_norm, p.qwidth, kFlatSplit).hi;
        if (lane == 0) thr[wave][qs] = t;
        dirty = true;
      }
      if (lane == qs) {
        cntv = cnt;
        wdv = wd;
        wiv = wi;
      }
    }
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
    // The consumer, a tile at a time: one compare, the eligibility bit and a ballot per accumulator register; the
    // registers with a candidate leave their ballot in the wave's LDS list and are settled in register order --
    // for any one query, over the tiles, that is ascending row order.  The thresholds a tile's insertions moved
    // are in the registers before the next tile's compares.
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if (t < ntiles && el[t] != 0) {
        const bool eligible = (el[t] >> col) & 1u;
        uint32_t pending = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = approx_distance<kIp>(qn[r], bn[t], c[t][r]);
          const uint64_t cm = __ballot(eligible && !(d > hi[r]));  // NaN: a candidate
          if (cm == 0ull) continue;
          if (lane == 0) pend[wave][r] = cm;
          pending |= 1u << r;
        }
        if (pending != 0) {
          wave_fence();
          while (pending != 0) {
            const int r = __builtin_ctz(pending);
            pending &= pending - 1;
            const uint64_t cm = uniform64(pend[wave][r]);
            const int qs = query_slot(0, r, 0);
#pragma unroll 1
            for (int hh = 0; hh < 2; ++hh) settle(qs + 4 * hh, sup + kTile * t, static_cast<uint32_t>(cm >> (32 * hh)));
          }
          wave_fence();
          if (dirty) {
#pragma unroll
            for (int r = 0; r < 16; ++r) hi[r] = thr[wave][query_slot(0, r, h)];
            dirty = false;
          }
        }
      }
    }
  }
  // the unused slots of the wave's lists, and its counters
#pragma unroll 1
  for (int qs = 0; qs < 32; ++qs) {
    const uint64_t qi = q0 + qs;
    if (qi >= p.nq) break;
    const uint32_t cnt = read_lane(cntv, qs);
    const uint64_t part = (chunk * p.nq + qi) * k;
    for (uint32_t e = cnt + lane; e < k; e += 64) {
      p.part_d[part + e] = FLT_MAX;
      p.part_i[part + e] = kEmptyId;
    }
  }
  if (lane == 0) {
    uint32_t *ws = p.wave_stats + (chunk * (nq_up / 32) + q0 / 32) * 2;
    ws[0] = st_verified;
    ws[1] = st_inserted;
  }
}

__global__ void __launch_bounds__(256) flat_filtered_mfma_reduce_kernel(const uint32_t *wave_stats, uint64_t waves,
                                                                        unsigned long long *stats) {
  reduce_wave_stats<2>(wave_stats, waves, stats);
}

__global__ void flat_filtered_mfma_clear_kernel(unsigned long long *stats) { clear_stats<2>(stats); }

// ---- host side -------------------------------------------------------------------------------------
FlatFilteredMfmaPlan flat_filtered_mfma_plan(uint64_t n, uint64_t nq, uint32_t k, uint32_t cus) {
  FlatFilteredMfmaPlan r{};
  k = std::min<uint32_t>(std::max<uint32_t>(k, 1), kFilteredMaxK);
  cus = std::max<uint32_t>(cus, 1);
  const uint64_t all = mfma_scan_queries_up(std::max<uint64_t>(nq, 1));
  r.sub_queries = all;
  if (n == 0) return r;
  // The shortest chunk: 1024 rows, or 32 k rows where that is more.  Every chunk starts with an empty list: its
  // first k eligible rows are verified and inserted whatever their distance, and until the first threshold
  // reaches the registers (one tile after the list fills) so is every eligible row; after that a list verifies
  // about k ln(rows / k) more when rows come in random order.  At 32 k rows the fill is 1/32 of the chunk and
  // the whole verify share about (1 + ln 32) / 32 = 0.14 of the rows; 1024 is the same rule at k = 32, below
  // which the 32-row tile, not k, is what the first threshold waits for.  Reasoned, not measured.
  const uint64_t min_rows = std::max<uint64_t>(1024, (32ull * k + kMfmaScanTileRows - 1) / kMfmaScanTileRows * kMfmaScanTileRows);
  const uint64_t list_bytes = static_cast<uint64_t>(k) * 8;
  const MfmaScanChunks c = mfma_scan_chunks(n, all, cus, min_rows, kFilteredPartialCap, [&](uint64_t) { return list_bytes; });
  r.chunk_rows = c.rows;
  r.chunks = (n + c.rows - 1) / c.rows;
  r.sub_queries = c.sub;
  r.partial_bytes = r.chunks * std::min<uint64_t>(std::max<uint64_t>(nq, 1), c.sub) * list_bytes;
  return r;
}

hipError_t launch_flat_filtered_mfma_prepare(const FlatFilteredMfmaParams &p, hipStream_t s) {
  if (p.nq == 0 || p.qwidth == 0 || p.qwidth % kMfmaScanKS != 0 || p.qwidth < p.dim) return hipErrorInvalidValue;
  const uint64_t nq_up = mfma_scan_queries_up(p.nq);
  hipLaunchKernelGGL(flat_filtered_mfma_prepare_kernel, dim3(static_cast<uint32_t>(nq_up / 4)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_flat_filtered_mfma_scan(const FlatFilteredMfmaParams &p, hipStream_t s) {
  const uint32_t grid = mfma_scan_grid(p.nq, p.n, p.chunk_rows, p.chunks, p.dim, p.stride, p.qwidth);
  if (grid == 0 || p.n > 0xffffffffull) return hipErrorInvalidValue;
  if (p.k == 0 || p.k > kFilteredMaxK) return hipErrorInvalidValue;
  if (p.ip)
    hipLaunchKernelGGL(flat_filtered_mfma_kernel<true>, dim3(grid), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(flat_filtered_mfma_kernel<false>, dim3(grid), dim3(256), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flat_filtered_mfma_reduce_kernel, dim3(1), dim3(256), 0, s, p.wave_stats,
                     p.chunks * (mfma_scan_queries_up(p.nq) / 32), p.stats);
  return hipGetLastError();
}

hipError_t launch_flat_filtered_mfma_clear(unsigned long long *stats, hipStream_t s) {
  hipLaunchKernelGGL(flat_filtered_mfma_clear_kernel, dim3(1), dim3(64), 0, s, stats);
  return hipGetLastError();
}

}  // namespace alaya_amd
