// What the three exact MFMA scans share on the device: flat_range_mfma_kernel (exact range search),
// flat_filtered_mfma_kernel (exact filtered k-NN) and flat_select_hist_kernel (k-NN by histogram selection).
// Device code only; the shape constants and the host's planner and launch check are in exact_scan_plan.h.
//
// The work split.  A workgroup of 4 waves owns kMfmaScanQueries = 128 queries (32 per wave) and one contiguous
// row chunk; the grid is XCD-aware as flat_scan_kernel's.
//
// The pass.  Rows stream through a double-buffered LDS unit of 32 rows x KS = 64 columns, split into bf16 hi + lo
// once when the unit is staged: x = hi + lo + a residual below 2^-16 |x|.  Per slab a wave splits its queries'
// slice into hi / lo A fragments (lane (col, h) holds query col, columns h KS/2 .. + KS/2 of the slab; the next
// slab's slice is in flight meanwhile) and runs a super-tile of TT = 4 tiles whose 32x32 accumulators
// (C[query][row]: row = lane & 31, query = query_slot(r, h) for register r) persist across the slabs: ql.bh +
// qh.bl + qh.bh, three v_mfma_f32_32x32x16_bf16 per 16 columns.  A tile has one eligibility word; a row past n or
// with a clear bit is streamed and contracted like any other and its result is dropped.  After the last slab a
// scan turns the accumulators into d~ = (|q|^2 + |b|^2) - 2 C (L2) or -C (IP) with approx_distance: the exactness
// arguments of all three scans (flat_range_bound.h) rest on that one operation order.
//
// KS = 64, TT = 4: a lane holds 64 accumulators, 32 VGPRs of A fragments, 32 of the next slab's f32 slice and 8
// of staging, beside what its consumer keeps; KS = 128 doubles the fragment and prefetch registers and would
// spill.  LDS reads: a wave reads 2 x 16 bytes per lane (bh, bl) per 3 MFMAs, 2 KiB per 96 MFMA cycles; 4 waves,
// 85 bytes per cycle of the CU's 128, whatever TT -- each B fragment feeds one wave's 3 MFMAs.  TT amortises
// what is per slab: the 8 float4 loads and the 32 hi/lo splits of the A slice, over TT x 12 MFMAs (1536 cycles
// at TT = 4), and the barrier per unit stays one per 12 MFMAs.
//
// The text of the pass itself -- the block map, load_a / load_unit / store_unit and the slab x tile loop -- is
// still written in each of the three kernels: as one function template here it compiles to other instructions
// (DESIGN.md "Round 28" has what was tried and what the compiler made of it), and a change of generated code is
// not a refactor.  Everything below compiles to the instructions of the text it replaced
// (profiles/r28/isa_compare.txt).
#pragma once
#include <hip/hip_runtime.h>

#include "exact_scan_plan.h"

namespace alaya_amd {
namespace mfma_scan {

constexpr int KS = kMfmaScanKS;
constexpr int TT = kMfmaScanTT;
constexpr int kTile = 32;
constexpr int kBPitch = KS + 8;          // bf16 per LDS row: 144 bytes, 16-byte reads spread over the banks
constexpr int kHalf = kTile * kBPitch;   // bf16 of one hi (or lo) unit
constexpr int kTileLds = 2 * 2 * kHalf;  // bf16 of the LDS tile buffers: two buffers of (hi unit, lo unit)
constexpr int kVecPerRow = KS / 4;
constexpr int kPerThread = kTile * kVecPerRow / 256;  // float4s of a unit per thread
static_assert(kTile * kVecPerRow % 256 == 0, "whole float4s per thread");
static_assert(kMfmaScanTileRows == kTile * TT, "a super-tile is TT tiles");

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split_bf16(float x, __bf16 &hi, __bf16 &lo) {
  hi = static_cast<__bf16>(x);
  lo = static_cast<__bf16>(x - static_cast<float>(hi));
}

__device__ __forceinline__ uint32_t read_lane(uint32_t v, int l) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), __builtin_amdgcn_readfirstlane(l)));
}
__device__ __forceinline__ float read_lane_f(float v, int l) {
  return __int_as_float(static_cast<int>(read_lane(static_cast<uint32_t>(__float_as_int(v)), l)));
}

// a value every lane holds alike, as a scalar
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  const uint32_t a = __builtin_amdgcn_readfirstlane(static_cast<int>(v));
  const uint32_t b = __builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32));
  return (static_cast<uint64_t>(b) << 32) | a;
}

__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The query that accumulator register r of a lane in half h belongs to, `first` being the wave's first query: as
// a slot of the wave with first = 0.
template <class T>
__device__ __forceinline__ T query_slot(T first, int r, int h) {
  return first + (r & 3) + 8 * (r >> 2) + 4 * h;
}

// d~ of a pair from |q|^2, |b|^2 and its accumulator
template <bool kIp>
__device__ __forceinline__ float approx_distance(float qn, float bn, float c) {
  return kIp ? -c : (qn + bn) - 2.0f * c;
}

// One workgroup of 256: the kSums per-wave counters of a scan launch added to the call's kSums sums.
template <int kSums>
__device__ __forceinline__ void reduce_wave_stats(const uint32_t *wave_stats, uint64_t waves, unsigned long long *stats) {
  __shared__ unsigned long long part[kSums][256];
  unsigned long long s[kSums] = {};
  for (uint64_t i = threadIdx.x; i < waves; i += 256)
    for (int j = 0; j < kSums; ++j) s[j] += wave_stats[i * kSums + j];
  for (int j = 0; j < kSums; ++j) part[j][threadIdx.x] = s[j];
  __syncthreads();
  if (threadIdx.x < kSums) {
    unsigned long long t = 0;
    for (int i = 0; i < 256; ++i) t += part[threadIdx.x][i];
    stats[threadIdx.x] += t;
  }
}

template <int kSums>
__device__ __forceinline__ void clear_stats(unsigned long long *stats) {
  if (threadIdx.x < kSums) stats[threadIdx.x] = 0;
}

}  // namespace mfma_scan
}  // namespace alaya_amd
