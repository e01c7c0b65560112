// C-ABI implementation (include/alaya_hip.h): device-resident index state, uploads, launches.
#include "../../include/alaya_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "build_kernels.h"
#include "extend_kernels.h"
#include "graph_update.h"
#include "hnsw_build.h"
#include "flat_bound.h"
#include "flat_filtered_kernels.h"
#include "flat_range_kernels.h"
#include "flat_kernels.h"
#include <cstdlib>
#include "screen_bound.h"
#include "search_kernels.h"

using alaya_amd::HostGraph;
using alaya_amd::SearchParams;

struct alaya_graph {
  HostGraph g;
};

namespace {

thread_local std::string g_last_error;

struct ArgError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

void hip_check(hipError_t e, const char *what) {
  if (e != hipSuccess) throw DeviceError(std::string(what) + ": " + hipGetErrorString(e));
}

template <typename F>
int guarded(F &&f) {
  try {
    f();
    return ALAYA_OK;
  } catch (const ArgError &e) {
    g_last_error = e.what();
    return ALAYA_ERR_ARG;
  } catch (const DeviceError &e) {
    g_last_error = e.what();
    return ALAYA_ERR_DEVICE;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return ALAYA_ERR_RUNTIME;
  }
}

// Grow-only device buffer.
struct DevBuf {
  void *ptr = nullptr;
  size_t bytes = 0;
  void reserve(size_t n) {
    if (n <= bytes) return;
    release();
    hip_check(hipMalloc(&ptr, std::max<size_t>(n, 256)), "hipMalloc");
    bytes = std::max<size_t>(n, 256);
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
  template <typename T>
  T *as() const {
    return static_cast<T *>(ptr);
  }
  ~DevBuf() { release(); }
};

uint32_t round_up32(uint32_t d) { return (d + 31u) / 32u * 32u; }

uint32_t ceil_log2(uint64_t v) {
  uint32_t l = 0;
  while ((1ull << l) < v) ++l;
  return l;
}

}  // namespace

struct alaya_index {
  int device = 0;
  std::mutex mu;
  // base
  uint64_t n = 0;
  uint32_t dim = 0, stride = 0;
  int metric = ALAYA_METRIC_L2;
  bool generic = false;  // ALAYA_DIST_GENERIC: non-float DataType rows, generic distance order
  DevBuf base, valid;
  bool has_valid = false;
  // graph
  bool has_graph = false;
  uint32_t R = 0, upper_R = 0, ep = 0, n_eps = 0;
  bool has_overlay = false, dedup = false;
  DevBuf l0, levels, upper_off, upper_edges, eps;
  uint64_t graph_n = 0;
  // SQ8 search space
  bool has_sq8 = false;
  int sq8_order = 2;
  uint32_t code_stride = 0;
  DevBuf codes, sq_min, sq_max, rr_q_buf, sq_ids, sq_d;
  // flat path
  DevBuf norms, cand_d, cand_i, flat_tau, flag_buf, iota, flat_q;
  DevBuf flat_bias;  // IP / COS: the scans' per-row bias, zeros in place of |b|^2 (ensure_norms)
  int flat_contraction = -1;  // the last flat search's: 0 = f32, 1 = bf16 hi/lo split, 2 = single-pass f16
  bool norms_ready = false;
  // single-role f16 flat scan: the base's tile records (alaya_amd::launch_flat_tiles), built at the
  // first flat search after any change to the rows, their count or the validity bitmap
  DevBuf flat_tiles, tiles_cand, tiles_qexp;  // the records; the scan's candidate buffers, query scales
  bool tiles_ready = false;
  int tiles_exp = 0;
  int tiles_metric = -1;  // the metric whose bias the records' tails carry
  float max_norm = 0.f;
  // scratch
  DevBuf work, overflow, dirty, stab, q_buf, id_buf, dist_buf, cnt_buf, dlist_buf, dout_buf;
  DevBuf allow_buf, group_buf;  // the host filtered search's masks and per-query mask indices
  DevBuf through_buf;           // the host through search's rows stepped through per query
  // range search: the append buffers of both entry points (nq x cap ids and distances, scratch between the search
  // launch and the sort), and the host entry's radii and counts
  DevBuf range_ids, range_d, range_radii, range_cnt;
  DevBuf range_cradii, range_cand;    // SQ8 range search, host entry: the code radii and the candidate counts
  DevBuf range_frontier, range_more;  // radius mode: nq x max_frontier frontier ids (scratch), the host entry's nq x 2 `more`
  // exact filtered scan (alaya_index_flat_search_filtered*): the current mask's id list (n words), the
  // compaction's block sums and count, the partial lists of one scan launch (capped, see
  // alaya_amd::flat_filtered_plan) and the queries ordered by mask
  DevBuf ff_ids, ff_sums, ff_count, ff_part_d, ff_part_i, ff_qlist;
  uint64_t ff_last[4] = {0, 0, 0, 0};  // alaya_index_flat_filtered_last
  // exact range search (alaya_index_flat_range_search*): it shares the filtered scan's id list, block sums,
  // count, query order and partial-list buffers; its own are the per-(chunk, query) hit counts and the
  // all-ones words that stand for "no mask" on an index without a validity bitmap
  DevBuf fr_part_n, fr_ones;
  uint64_t fr_last[6] = {0, 0, 0, 0, 0, 0};  // alaya_index_flat_range_last
  size_t overflow_clean = 0;  // leading bytes of `overflow` known to be zero (kernels leave it clean)
  size_t stab_clean = 0;      // the same for the spill tables
  uint32_t hash_log2_override = 0;
  int helpers_mode = -1;          // distance helpers: -1 automatic, 0 off, 1 on (alaya_index_set_helpers)
  DevBuf help_stats;              // per searcher of the last helper launch: (memo distances, memo expansions)
  uint64_t help_stats_slots = 0;
  // candidate screen of the wide-row f32 L2 graph search, one copy of the base per format
  // (SearchParams::screen): [0] the rows as f16 and, per row, an upper bound on ||x - f16(x)||
  // (alaya_amd::launch_screen_rows); [1] the 8-bit records, `err` unused
  // (alaya_amd::launch_screen_rows_u8).  Each is built at the first search that uses its format,
  // kept current by row writes, freed with the base it describes.
  struct ScreenCopy {
    DevBuf rows, err;
    uint64_t cap = 0;     // rows the buffers hold
    bool ready = false;   // rows [0, n) are current
    bool failed = false;  // the buffers could not be allocated for this base: plain kernel
  };
  ScreenCopy screen_copy[2];
  uint32_t screen_format = 0;     // SearchParams::screen of the launch being planned (ensure_screen)
  DevBuf screen_stats;
  uint64_t screen_stats_slots = 0;  // searchers of the last launch, 0 = it did not screen
  uint32_t last_grid = 0, last_waves = 0;  // the last search launch's workgroups and waves per workgroup
  // the rest of its plan (alaya_index_last_plan): LDS bytes per workgroup, visited-table log2 slots and
  // layout, searchers per CU, SearchParams::scout
  uint32_t last_lds = 0, last_hash_log2 = 0, last_compact = 0, last_per_cu = 0, last_scout = 0;
  DevBuf scout_stats;
  uint64_t scout_stats_slots = 0;   // searchers of the last launch, 0 = it had no scouts
  DevBuf scout_policy_stats;        // (the same slots)
  uint32_t last_scout_policy = 0;   // SearchParams::scout_policy of the last launch
  int visited_mode_override = 0;  // 0 auto, 1 compact 16-bit slots, 2 wide 32-bit slots,
                                  // 3 compact with probes capped at 2 (exercises the probe spill)
  int num_cus = 0;
  // online updates (alaya_index_enable_updates): host mirror + JobContext, device capacity
  uint64_t capacity = 0;
  std::unique_ptr<alaya_amd::HostGraph> upd_graph;
  std::unique_ptr<alaya_amd::RowMirror> upd_rows;
  std::unique_ptr<alaya_amd::UpdateContext> upd_ctx;
  hipStream_t stream = nullptr;
  // Per-index scratch (work counter, visited spill area, flat candidates, SQ8 id buffer) is shared
  // by every launch; `scratch_ev` marks the end of the last launch that used it, on
  // `scratch_stream`.  A launch on another stream waits for it first (scratch_acquire), and calls
  // that replace or free device buffers drain it (scratch_drain).
  hipEvent_t scratch_ev = nullptr;
  hipStream_t scratch_stream = nullptr;
  bool scratch_used = false;
  uint64_t device_bytes() const {
    return base.bytes + valid.bytes + l0.bytes + levels.bytes + upper_off.bytes +
           upper_edges.bytes + eps.bytes + overflow.bytes + dirty.bytes + stab.bytes + codes.bytes + sq_min.bytes +
           sq_max.bytes;
  }
};

namespace {

void set_device(const alaya_index *ix) { hip_check(hipSetDevice(ix->device), "hipSetDevice"); }

// Order this call's launches on `s` after every earlier launch that used the index's scratch.
void scratch_acquire(alaya_index *ix, hipStream_t s) {
  if (ix->scratch_used && ix->scratch_stream != s)
    hip_check(hipStreamWaitEvent(s, ix->scratch_ev, 0), "hipStreamWaitEvent");
}
// Mark the end of this call's launches on `s`.
void scratch_release(alaya_index *ix, hipStream_t s) {
  hip_check(hipEventRecord(ix->scratch_ev, s), "hipEventRecord");
  ix->scratch_stream = s;
  ix->scratch_used = true;
}
// The visited spill areas (bitsets, spill tables) are zeroed once and then kept clean by every
// query that finishes.  A launch or sync that reports an error may have left a query half done, so
// the next launch zeroes them again.
void scratch_suspect(alaya_index *ix) {
  ix->overflow_clean = 0;
  ix->stab_clean = 0;
}
// Wait (host side) until no launch can still read or write the index's device buffers.
void scratch_drain(alaya_index *ix) {
  if (!ix->scratch_used) return;
  const hipError_t e = hipEventSynchronize(ix->scratch_ev);
  if (e != hipSuccess) scratch_suspect(ix);
  hip_check(e, "hipEventSynchronize");
}
// guarded() for the entry points that launch searches on the index's scratch: a device error marks
// the spill areas for re-zeroing.  This covers errors the call itself sees (launch failures, and the
// synchronous entry points' syncs, scratch_drain).  A stream-async *_device call returns before its
// kernel ends; a fault surfacing later (at a torch sync) is not seen here.  HIP errors from a device
// fault are sticky -- the context is unusable and every later call of this index throws -- so no
// later launch runs on tables a half-finished query left dirty.
template <typename F>
int guarded_scratch(alaya_index *ix, F &&f) {
  return guarded([&] {
    try {
      f();
    } catch (const DeviceError &) {
      if (ix) scratch_suspect(ix);
      throw;
    }
  });
}

SearchParams base_params(alaya_index *ix) {
  SearchParams p{};
  p.base = ix->base.as<float>();
  p.n = ix->n;
  p.dim = ix->dim;
  p.stride = ix->stride;
  p.valid = ix->has_valid ? ix->valid.as<uint32_t>() : nullptr;
  p.ip = ix->metric != ALAYA_METRIC_L2;
  p.generic = ix->generic;
  return p;
}

constexpr size_t kLdsPerCu = 160 * 1024;
constexpr uint32_t kDirtyCap = 16384;  // per-slot dirty-word list (64 KB): words a spilled query set

// Spill table size (log2 entries per slot) for an AVX-512-order SQ8 search, 0 = the bitset is the
// second level.
// ~32 ef entries (config 5, ef 340: 2^14 = 32 KB per slot for ~2.7k visited ids, load 0.16, so a
// full bucket of 8 -- the bitset fallback -- is rare); at least 2^(L - 12) so an entry (1 + the
// hash's low L - (s - 3) bits) fits 16 bits; at most 2^16 (128 KB per slot; ids wider than 28 bits
// keep the bitset).  ALAYA_SPILL_TABLE=0 keeps the bitset, a value 6..16 forces the size (tests: tiny
// tables fill their buckets and exercise the bitset fallback).
uint32_t spill_table_log2(int sq8_order, uint32_t L, uint32_t ef) {
  // f32 kernels keep the LDS first level and the bitset (their tables rarely spill; on the spill
  // table SIFT ran 23 % slower); so do the AVX2-order SQ8 kernels (hosts without AVX-512), whose
  // SGPR budget the table's state would overrun (65-116 restores per expansion)
  if (sq8_order != 2) return 0;
  uint32_t s = std::max<uint32_t>({6u, ceil_log2(32ull * ef), L > 12 ? L - 12 : 0u});
  if (const char *e = std::getenv("ALAYA_SPILL_TABLE")) {
    const uint32_t v = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
    if (v == 0) return 0;
    if (v >= 6 && v <= 16) s = v;
  }
  s = std::min<uint32_t>(s, L + 3);  // buckets <= 2^L: the bucket index is the hash's top bits
  if (s > 16 || s < 6 || L - (s - 3) > 15) return 0;
  return s;
}

// The visited set's second level for `slots` persistent searchers over ix->n rows: one clean N-bit
// bitset per slot (zeroed once when allocated; every query leaves it clean) and a dirty-word list,
// plus (SQ8 searches, spill_table_log2) one clean spill table per slot.
void prepare_spill(alaya_index *ix, SearchParams &p, uint64_t slots, hipStream_t stream) {
  const uint64_t words = (ix->n + 31) / 32;
  const size_t bytes = static_cast<size_t>(std::max<uint64_t>(slots, 1)) * words * 4;
  if (bytes > ix->overflow.bytes) {
    ix->overflow.reserve(bytes);
    ix->overflow_clean = 0;
  }
  if (ix->overflow_clean < ix->overflow.bytes) {
    hip_check(hipMemsetAsync(ix->overflow.ptr, 0, ix->overflow.bytes, stream), "hipMemsetAsync");
    ix->overflow_clean = ix->overflow.bytes;
  }
  uint32_t cap = kDirtyCap;
  if (const char *e = std::getenv("ALAYA_DIRTY_CAP")) cap = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));  // tests
  ix->dirty.reserve(static_cast<size_t>(std::max<uint64_t>(slots, 1)) * std::max<uint32_t>(cap, 1) * 4);
  p.overflow_bits = ix->overflow.as<uint32_t>();
  p.dirty_words = ix->dirty.as<uint32_t>();
  p.dirty_cap = cap;
  p.spill_table = nullptr;
  p.stab_rbits = 0;
  p.spill_flags = 0;
  if (const char *e = std::getenv("ALAYA_SPILL_FLAGS")) p.spill_flags = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
  if (const uint32_t st = p.stab_log2) {
    const size_t tbytes = static_cast<size_t>(std::max<uint64_t>(slots, 1)) * (2ull << st);
    if (tbytes > ix->stab.bytes) {
      ix->stab.reserve(tbytes);
      ix->stab_clean = 0;
    }
    if (ix->stab_clean < ix->stab.bytes) {
      hip_check(hipMemsetAsync(ix->stab.ptr, 0, ix->stab.bytes, stream), "hipMemsetAsync");
      ix->stab_clean = ix->stab.bytes;
    }
    const uint32_t rbits = p.vis_lbits - (st - 3);
    p.spill_table = ix->stab.as<uint16_t>();
    p.stab_log2 = st;
    p.stab_rbits = rbits;
  }
}

// Waves per search workgroup: SQ8 searchers share the quantizer's per-dimension scale and min
// (search_shared_lds_bytes) across 4 waves, one per SIMD; f32 searchers have nothing to share.
// ALAYA_SEARCH_WAVES overrides (1, 2 or 4; diagnostics).
int search_waves(const SearchParams &p) {
  if (const char *e = std::getenv("ALAYA_SEARCH_WAVES")) {
    const int w = std::atoi(e);
    if (w == 1 || w == 2 || w == 4) return w;
  }
  return p.sq8_order != 0 ? 4 : 1;
}

// Size the LDS visited table for residency: the batch wants ceil(nq / CUs) resident queries
// (waves) per CU; the register file caps that.  With more queries than resident slots the launch
// runs as many waves as the registers admit -- a spill to the global second level is one atomicOr
// per visit and no clearing beyond the words set (visit_end), so residency beats table size
// (config 5, 10k queries: 4 -> 8 -> 12 waves per CU with 16 / 8 / 4 KB tables took 20.3 / 13.3 /
// 11.1 ms; profiles/r03/sweeps) -- and the table takes what LDS is left per wave at that count
// (workgroups of W waves plus the shared region), never below 256 slots, never more than ~2x the
// expected visited count (48 ef).  Layout: compact 16-bit slots (twice the entries per byte)
// whenever the ids' hash remainder fits (log2 n - log2 slots <= 11), else 32-bit id slots.
// Returns log2 slots; sets p.vis_*.
constexpr uint32_t kMaxCompactRbits = 11;
// At most 4 searchers per SIMD: a 5th wave (the 96-VGPR d = 128 L2 kernel admits 5) halves every
// table and costs more in probes than it hides -- SIFT 1M, 10k queries, ef 70: 16 waves per CU with
// 4096-slot tables 1.198 ms, 20 with 2048-slot tables 1.513 ms (profiles/r03/sift_c3/residency_sweep_tree.log);
// config 5 measured 12 and 16 per CU equal.
constexpr uint64_t kMaxSearchWavesPerCu = 16;
uint64_t max_search_waves_per_cu() {
  if (const char *e = std::getenv("ALAYA_MAX_WAVES_PER_CU"))  // diagnostics (tools/shape_sweep.py)
    return std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
  return kMaxSearchWavesPerCu;
}

// Distance helpers (search kernel kModeHelp, search_has_helpers): with helpers every search runs 4-wave
// workgroups, and a batch smaller than the resident searchers still fills the CUs, so each workgroup
// has idle waves to help from the start.  Automatic policy, from the measurements in DESIGN.md
// (round 5, "distance helpers"): on for the SQ8 kernels (config 5: 1k queries 3.75 -> 3.54 ms, 10k
// 9.60 -> 9.53 ms); for the small-row f32 kernels only when the batch outnumbers the resident
// searchers, i.e. for its tail (SIFT-shaped 10k 1.192 -> 1.138 ms; at 1k the helper layout costs more
// than it saves: 0.536 -> 0.583 ms).  alaya_index_set_helpers and ALAYA_HELPERS=0/1 override it.
bool helpers_requested(const alaya_index *ix, const SearchParams &p, uint64_t nq, uint64_t cus) {
  if (const char *e = std::getenv("ALAYA_HELPERS")) return std::atoi(e) != 0;  // A/B override
  if (ix->helpers_mode >= 0) return ix->helpers_mode > 0;
  if (std::getenv("ALAYA_SEARCH_WAVES")) return false;  // a forced workgroup shape (diagnostics, tests)
  if (p.sq8_order == 2) return true;
  return nq > max_search_waves_per_cu() * cus;
}

// filter_k != 0: the filtered search -- its own kernel's registers, and a result pool of filter_k entries
// in every wave's region (hop: the through search's kernel).  range: the range search -- its own kernel's
// registers and no result pool (more: its radius mode's kernel).
uint32_t size_visited(alaya_index *ix, SearchParams &p, const alaya_amd::SearchVariant &v, uint64_t nq, uint32_t ef,
                      int W = 1, uint32_t filter_k = 0, bool hop = false, bool range = false, bool more = false) {
  const uint32_t lbits = std::max<uint32_t>(1, ceil_log2(std::max<uint64_t>(ix->n, 2)));
  const int mode = ix->visited_mode_override;  // 0 auto, 1 compact, 2 wide, 3 compact + short probes
  auto set_mode = [&](uint32_t l, bool compact) {
    p.vis_lbits = lbits;
    p.vis_rbits = compact ? (lbits > l ? lbits - l : 0u) : alaya_amd::kVisWide;
    p.vis_max_disp = compact ? (0xffffu >> p.vis_rbits) - 1u : 0u;
    if (compact && mode == 3) p.vis_max_disp = std::min<uint32_t>(p.vis_max_disp, 2u);
    p.vis_limit = 0u;
    if (const char *e = std::getenv("ALAYA_VIS_LIMIT_PCT")) {  // diagnostics: spill threshold in % of slots
      const uint64_t slots = 1ull << l;
      const uint64_t lim = slots * std::min<uint64_t>(100, std::strtoull(e, nullptr, 10)) / 100;
      // exact at any threshold up to slots - 64: one visit inserts at most 64 ids, and a compact
      // probe past max_disp spills by itself
      p.vis_limit = static_cast<uint32_t>(std::max<uint64_t>(64, std::min<uint64_t>(lim, slots - 64)));
    }
    if (const char *e = std::getenv("ALAYA_VIS_LIMIT")) {  // diagnostics: spill threshold in entries (1 = at the
      const uint64_t lim = std::strtoull(e, nullptr, 10);  // first expansion); exact up to slots - 64
      if (lim > 0) p.vis_limit = static_cast<uint32_t>(std::min<uint64_t>(lim, (1ull << l) - 64));
    }
    return l;
  };
  auto fits_compact = [&](uint32_t l) { return (lbits > l ? lbits - l : 0u) <= kMaxCompactRbits; };
  if (ix->hash_log2_override) {
    const uint32_t l = ix->hash_log2_override;
    const bool compact = mode == 1 || mode == 3 || (mode == 0 && fits_compact(l));
    if (compact && !fits_compact(l)) throw ArgError("compact visited table cannot encode ids of this index");
    return set_mode(l, compact);
  }
  if (p.stab_log2 != 0 && mode != 1 && mode != 3) {
    // The spill table is the second level: a query spills at its first expansion into a 128-slot
    // first level, then every visit is prefetched bucket reads (config 5: 10k queries 9.30 ->
    // 9.20 ms, 1k queries 3.89 -> 3.69 ms against first levels sized for LDS;
    // profiles/r04/spill_table/c5_first_level_size_threshold.log).  LDS then bounds nothing.
    return set_mode(7, false);
  }
  const size_t shared = alaya_amd::search_shared_lds_bytes(ix->stride, p.sq8_order != 0) +
                        (p.help ? alaya_amd::kHelpBoardBytes : 0);
  const size_t wave_fixed = alaya_amd::search_wave_lds_bytes(ix->stride, ef, 0, false, p.sq8_order) - 4 +
                            (filter_k ? alaya_amd::filter_result_lds_bytes(filter_k) : 0);
  // the register-bound residency, probed with a 4 KB table.  The 1 KB probe applies only to the
  // forced compact modes (1, 3) with a spill table: every other mode with a spill table returned
  // set_mode(7) above.
  const bool stab = p.stab_log2 != 0;  // set by do_search (spill_table_log2)
  int vgpr_blocks = 0;
  const size_t probe_lds = shared + W * (wave_fixed + (stab ? 1024 : 4096));
  hip_check(more    ? alaya_amd::range_more_search_occupancy(ix->dim, ix->generic, p.ip, W, probe_lds, &vgpr_blocks)
            : range && p.sq8_order
                ? alaya_amd::range_sq8_search_occupancy(ix->dim, p.sq8_order, p.ip, W, probe_lds, &vgpr_blocks)
            : range ? alaya_amd::range_search_occupancy(ix->dim, ix->generic, p.ip, W, probe_lds, &vgpr_blocks)
            : !filter_k ? alaya_amd::search_occupancy(v, p.ip, W, probe_lds, &vgpr_blocks)
            : hop ? alaya_amd::filtered_hop_search_occupancy(ix->dim, ix->generic, p.ip, W, probe_lds, &vgpr_blocks)
            : p.sq8_order ? alaya_amd::filtered_sq8_search_occupancy(ix->dim, p.sq8_order, p.ip, W, probe_lds, &vgpr_blocks)
                          : alaya_amd::filtered_search_occupancy(ix->dim, ix->generic, p.ip, W, probe_lds, &vgpr_blocks),
            "occupancy");
  const uint64_t vgpr_waves = static_cast<uint64_t>(std::max(1, vgpr_blocks)) * W;
  const uint64_t max_waves = std::max<uint64_t>(W, max_search_waves_per_cu());
  // with helpers a small batch still fills the CUs (the waves without a query help)
  const uint64_t want = p.help ? max_waves : (nq + ix->num_cus - 1) / std::max(1, ix->num_cus);
  uint64_t waves = std::max<uint64_t>(1, std::min<uint64_t>({vgpr_waves, want, max_waves}));
  const uint32_t cap = ceil_log2(48ull * ef);
  // table bytes per wave when `w` waves share a CU in workgroups of W
  auto table_budget = [&](uint64_t w) -> size_t {
    const uint64_t blocks = std::max<uint64_t>(1, w / W);
    const size_t per_block = kLdsPerCu / blocks;
    if (per_block <= shared) return 0;
    const size_t per_wave = (per_block - shared) / W;
    return per_wave > wave_fixed ? per_wave - wave_fixed : 0;
  };
  const size_t min_table = (mode == 2 || !fits_compact(9)) ? (4u << 8) : (2u << 9);  // 256 wide / 512 compact slots
  while (waves > static_cast<uint64_t>(W) && table_budget(waves) < min_table) waves -= W;
  const size_t budget = table_budget(waves);
  auto pick = [&](size_t slot_bytes, uint32_t lmax) {
    uint32_t l = 8;
    while (l < lmax && (slot_bytes << (l + 1)) <= budget) ++l;
    return std::max<uint32_t>(8, std::min<uint32_t>(l, cap));
  };
  if (mode == 0) {
    // a 32-bit id table of >= 32 ef slots (load <= ~0.3 at the usual 10-24 visited ids per ef)
    // costs one LDS atomic per probe instead of a load and a compare-and-swap: where it fits (the
    // 1k-query SIFT shape) it is 11 % faster; a compact table stays the choice when LDS is short
    const uint32_t wl = std::max<uint32_t>(10, ceil_log2(32ull * ef));
    if (wl <= 15 && (static_cast<size_t>(4) << wl) <= budget) return set_mode(wl, false);
  }
  if (mode != 2) {
    const uint32_t l = pick(2, 16);
    if (fits_compact(l)) return set_mode(l, true);
    if (mode == 1 || mode == 3) throw ArgError("compact visited table cannot encode ids of this index");
  }
  return set_mode(pick(4, 15), false);
}

// CUs a launch on `s` may use: all of the device's, unless the stream carries a CU mask
// (alaya_stream_create_reserving: the persistent grid is sized to the CUs left to it, so none of its
// workgroups waits for a CU that another stream's kernels -- the shard exchange's -- keep).
int stream_cus(const alaya_index *ix, hipStream_t s) {
  if (s == nullptr) return ix->num_cus;
  uint32_t mask[32] = {};
  const uint32_t words = static_cast<uint32_t>((ix->num_cus + 31) / 32);
  if (words > 32 || hipExtStreamGetCUMask(s, words, mask) != hipSuccess) {
    (void)hipGetLastError();
    return ix->num_cus;
  }
  int c = 0;
  for (uint32_t w = 0; w < words; ++w) c += __builtin_popcount(mask[w]);
  return c > 0 && c <= ix->num_cus ? c : ix->num_cus;
}

bool ensure_screen(alaya_index *ix, const SearchParams &p, bool eligible, hipStream_t stream);

// What policy wants of a search's kernel: the features (kMode bits, search_variants.h) of one launch,
// decided in the order they depend on each other -- stamps and the prefetch check come with the
// call, helpers rule out two waves, and any of those but the check rules out the screen.
alaya_amd::SearchRequest search_request(alaya_index *ix, const SearchParams &p, uint64_t nq, uint32_t ef,
                                        hipStream_t stream) {
  using namespace alaya_amd;
  SearchRequest r{ix->dim, p.ip, p.sq8_order, ix->generic, p.stamps != nullptr ? kModeStamp : 0};
  // diagnostics flags (prepare_spill hands them to the kernel); bit 8 asks for the prefetch-check kernel
  if (const char *e = std::getenv("ALAYA_SPILL_FLAGS"))
    if ((std::strtoul(e, nullptr, 10) & 256u) != 0) r.want |= kModeCheck;
  // distance helpers (4-wave workgroups; a helper's memo of 4 x R entries lives in its pool and
  // visited table, checked by plan_search)
  if (helpers_requested(ix, p, nq, static_cast<uint64_t>(stream_cus(ix, stream))) && ix->R <= 64 &&
      search_has_helpers(ix->dim, p.sq8_order, ix->generic))
    r.want |= kModeHelp;
  // Wide f32 rows (d = 768 / 960) run one searcher per SIMD; a batch a little larger than that
  // (config 4's S = 1 layout: 1,250 queries per rank on 1,024 searchers) would leave most of a
  // second round idle, so it runs the two-waves-per-SIMD kernel instead (one row per lane group):
  // GIST-shaped 1M, ef 373, 1,250 queries 8.92 -> 7.44 ms, <= 1,024 queries equal, 2,048 and more
  // slower (profiles/r05/gist_rounds/).  ALAYA_TWO_WAVES = 0 / 1 forces it off / on.
  const bool plain = (r.want & (kModeHelp | kModeStamp)) == 0;
  if (plain && search_has_two_waves(ix->dim, p.sq8_order, ix->generic)) {
    const char *e = std::getenv("ALAYA_TWO_WAVES");
    const int force = e ? std::atoi(e) : -1;
    if (force == 1) {
      r.want |= kModeTwoWaves;
    } else if (force != 0) {
      int b1 = 0;  // resident searchers of the one-wave kernel: the request as it stands
      const size_t probe = search_wave_lds_bytes(ix->stride, ef, 12, true);
      hip_check(search_occupancy(resolve_search_variant(r), p.ip, 1, probe, &b1), "occupancy");
      const uint64_t resident1 = static_cast<uint64_t>(std::max(1, b1)) * static_cast<uint64_t>(stream_cus(ix, stream));
      if (nq > resident1 && 2 * nq <= 3 * resident1) r.want |= kModeTwoWaves;
    }
  }
  // candidate screen on an f16 row copy (wide f32 L2 rows), built here at the first launch that screens
  if (ensure_screen(ix, p, p.sq8_order == 0 && plain, stream)) r.want |= kModeScreen;
  return r;
}

// One search launch: the kernel variant its request resolved to and the shape sized for that kernel.
struct SearchPlan {
  const alaya_amd::SearchVariant *variant;
  int W;       // waves (searchers) per workgroup
  size_t lds;  // bytes per workgroup
  int grid;    // persistent workgroups
  int per_cu;  // resident workgroups per CU
};

// ALAYA_SEARCH_SCOUT (0 = off, 1 = on, 2 = on and every memo hit verified against the searcher's own
// bounds; unset = scout_default) and the diagnostics flag ALAYA_SEARCH_SCOUT_MISS=1 (no answer ever
// matches: every expansion takes the fallback) as SearchParams::scout.
// Default per width: on where the scouted search measured faster on MI355X than the same launch
// without scouts, and than the parent build, by the project's rule (the slowest new run above the
// fastest old one by more than 3x the old one's min-max spread): d = 768 and d = 960, GIST-shaped, 1k
// queries.  The runs and their figures are in profiles/r11/README.md and DESIGN.md section 3, "Round 11".
uint32_t scout_default(uint32_t dim) { return (dim == 768 || dim == 960) ? alaya_amd::kScoutOn : 0u; }

uint32_t scout_requested(uint32_t dim) {
  const char *e = std::getenv("ALAYA_SEARCH_SCOUT");
  const int asked = e && e[0] ? std::atoi(e) : -1;
  uint32_t f = asked < 0 ? scout_default(dim) : (asked == 1 ? alaya_amd::kScoutOn : (asked == 2 ? alaya_amd::kScoutOn | alaya_amd::kScoutVerify : 0u));
  if (f != 0u) {
    const char *m = std::getenv("ALAYA_SEARCH_SCOUT_MISS");
    if (m && std::atoi(m) != 0) f |= alaya_amd::kScoutMiss;
  }
  return f;
}

// ALAYA_SEARCH_SCOUT_POLICY (a mask of kScoutEarly = 1 and kScoutRecheck = 2; unset =
// scout_policy_default) as SearchParams::scout_policy of a scouted launch.
// Default per width: the bits that measured faster on MI355X by the project's rule -- the early
// request against the same launch without it, the second look beside the early request against the
// early request alone (on its own it returns a fifth of the scouts' records and no time) -- at d = 960
// and d = 768 alike (profiles/r12/README.md, DESIGN.md section 3, "Round 12").
uint32_t scout_policy_default(uint32_t dim) {
  return (dim == 768 || dim == 960) ? (alaya_amd::kScoutEarly | alaya_amd::kScoutRecheck) : 0u;
}

uint32_t scout_policy_requested(uint32_t dim) {
  const char *e = std::getenv("ALAYA_SEARCH_SCOUT_POLICY");
  if (!(e && e[0])) return scout_policy_default(dim);
  return static_cast<uint32_t>(std::strtoul(e, nullptr, 0)) &
         (alaya_amd::kScoutEarly | alaya_amd::kScoutRecheck);
}

// Resolves the request and sizes the launch for the kernel it got, so a feature that has no kernel
// for this shape is planned as absent: sets p.help / p.two_waves / p.screen, the visited table
// (p.hash_log2, p.vis_*), p.wave_lds and p.memo_off.  A stamped call whose shape has no stamped
// kernel is an error (its stamps would all be zero).
SearchPlan plan_search(alaya_index *ix, SearchParams &p, alaya_amd::SearchRequest r, uint64_t nq, uint32_t ef,
                       hipStream_t stream) {
  using namespace alaya_amd;
  SearchPlan plan{};
  // waves per workgroup: never more than the batch needs (helpers: always 4).  A plan with helpers
  // that does not fit (the memo, or four waves' LDS with a forced large visited table) falls back
  // to the search without them.
  for (;;) {
    plan.variant = &resolve_search_variant(r);
    const int mode = plan.variant->mode;
    if ((r.want & kModeStamp) != 0 && (mode & kModeStamp) == 0)
      throw ArgError("no stamped search kernel for dim " + std::to_string(ix->dim) +
                     (p.sq8_order ? " SQ8 (order " + std::to_string(p.sq8_order) + ")" : std::string(" f32")) +
                     ": see the variant list in search_variants.h");
    p.help = (mode & kModeHelp) != 0;
    p.two_waves = (mode & kModeTwoWaves) != 0;
    p.screen = (mode & kModeScreen) != 0 ? ix->screen_format : 0u;
    plan.W = p.help ? 4 : search_waves(p);
    while (!p.help && plan.W > 1 && static_cast<uint64_t>(plan.W) > nq) plan.W /= 2;
    p.hash_log2 = size_visited(ix, p, *plan.variant, nq, ef, plan.W);
    const bool compact = p.vis_rbits != kVisWide;
    p.wave_lds = static_cast<uint32_t>(search_wave_lds_bytes(ix->stride, ef, p.hash_log2, compact, p.sq8_order));
    bool fits = true;
    if (p.help) {
      // the memo (W searchers x kHelpMemoSlots requests x R entries of 8 bytes) overlays the memo
      // wave's query vector, or else its pool and visited table (past the query and the three
      // 64-entry lists the helper still uses)
      const size_t need = static_cast<size_t>(plan.W) * kHelpMemoSlots * ix->R * 8;
      const size_t q_bytes = search_query_lds_bytes(ix->stride, p.sq8_order);
      if (q_bytes >= need) {
        p.memo_off = 0;
      } else if (p.wave_lds >= q_bytes + 3 * 64 * 4 + need) {
        p.memo_off = static_cast<uint32_t>(q_bytes + 3 * 64 * 4);
      } else {
        fits = false;
      }
    }
    plan.lds = search_shared_lds_bytes(ix->stride, p.sq8_order != 0) + static_cast<size_t>(plan.W) * p.wave_lds +
               (p.help ? kHelpBoardBytes : 0);
    if (!p.help || (fits && plan.lds <= kLdsPerCu)) break;
    r.want &= ~kModeHelp;
  }
  if (plan.lds > kLdsPerCu) throw ArgError("ef / dim too large for the LDS budget");
  int per_cu = 0;
  hip_check(search_occupancy(*plan.variant, p.ip, plan.W, plan.lds, &per_cu), "occupancy");
  per_cu = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(per_cu, max_search_waves_per_cu() / plan.W)));
  // with helpers the grid fills the CUs whatever the batch (idle waves help from the start)
  const uint64_t cus = static_cast<uint64_t>(stream_cus(ix, stream));
  const uint64_t blocks_needed = p.help ? static_cast<uint64_t>(per_cu) * cus : (nq + plan.W - 1) / plan.W;
  plan.grid = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(blocks_needed, static_cast<uint64_t>(per_cu) * cus)));
  plan.per_cu = per_cu;
  // Scout: a launch that would run the one-wave kernel under the integer screen at d = 768 / 960, one
  // searcher per workgroup, moves to the two-waves kernel with a scout wave beside every searcher --
  // the second wave per SIMD that the batch leaves idle.  Only if nothing else changes: the visited
  // table and the searcher's LDS region are the ones planned above, the board fits beside them without
  // costing a resident workgroup, and the batch runs in one round (a larger batch's second wave per
  // SIMD belongs to another searcher).  Otherwise the plan stands as it is: never half on.
  p.scout = 0u;
  p.scout_policy = 0u;
  const uint32_t scout = scout_requested(ix->dim);
  if (scout != 0u && p.screen == 3u && !p.ip && !p.two_waves && !p.help && plan.W == 1 && ix->R <= kScoutR &&
      (plan.variant->mode & ~kModeScreen) == 0 && search_has_two_waves(ix->dim, p.sq8_order, ix->generic) &&
      !helpers_requested(ix, p, nq, cus)) {
    SearchRequest r2 = r;
    r2.want |= kModeTwoWaves;
    const SearchVariant &v2 = resolve_search_variant(r2);
    const size_t lds2 = plan.lds + kScoutBoardBytes;
    int per_cu2 = 0;
    if (v2.mode == (kModeScreen | kModeTwoWaves) && lds2 <= kLdsPerCu)
      hip_check(search_occupancy(v2, false, 2, lds2, &per_cu2), "occupancy");
    if (per_cu2 >= per_cu && nq <= static_cast<uint64_t>(per_cu) * cus) {
      plan.variant = &v2;
      plan.lds = lds2;
      p.scout = scout;
      p.scout_policy = scout_policy_requested(ix->dim);
      // diagnostics (ALAYA_SEARCH_SCOUT_GRID, include/alaya_hip.h): fewer workgroups than queries, so every
      // searcher -- and its scout -- runs several queries of the launch, one after the other
      if (const char *e = std::getenv("ALAYA_SEARCH_SCOUT_GRID"))
        plan.grid = std::max(1, std::min(plan.grid, std::atoi(e)));
    }
  }
  return plan;
}

// base_params plus the graph and one batch: what every graph search launch reads and writes.
SearchParams graph_search_params(alaya_index *ix, const float *d_q, uint64_t nq, uint32_t k, uint32_t ef, uint32_t *d_ids,
                                 float *d_dists, uint32_t *d_cnt) {
  SearchParams p = base_params(ix);
  p.l0 = ix->l0.as<uint32_t>();
  p.R = ix->R;
  p.dedup_edges = ix->dedup;
  p.levels = ix->has_overlay ? ix->levels.as<uint32_t>() : nullptr;
  p.upper_off = ix->upper_off.as<uint64_t>();
  p.upper_edges = ix->upper_edges.as<uint32_t>();
  p.upper_R = ix->upper_R;
  p.ep = ix->ep;
  p.eps = ix->eps.as<uint32_t>();
  p.n_eps = ix->n_eps;
  p.queries = d_q;
  p.nq = nq;
  p.q_stride = ix->dim;
  p.k = k;
  p.ef = ef;
  p.out_ids = d_ids;
  p.out_dists = d_dists;
  p.out_counters = d_cnt;
  return p;
}

// The search space of one launch: the SQ8 codes with their scale and min (sq8; the caller has checked
// ix->has_sq8), and the visited second level that goes with the space -- spill table or bitset.
void set_search_space(alaya_index *ix, SearchParams &p, bool sq8, uint32_t ef) {
  if (sq8) {
    p.sq8_order = ix->sq8_order;
    p.codes = ix->codes.as<uint8_t>();
    p.code_stride = ix->code_stride;
    p.sq_min = ix->sq_min.as<float>();
    p.sq_max = ix->sq_max.as<float>();
  }
  p.stab_log2 = spill_table_log2(p.sq8_order, std::max<uint32_t>(1, ceil_log2(std::max<uint64_t>(ix->n, 2))), ef);
}

// Records the plan of the launch about to go out (alaya_index_last_launch / _last_plan, and which of the
// scout, helper and screen counters its `searchers` will have written) and resets the work counter.
void record_launch(alaya_index *ix, SearchParams &p, int grid, int wg_waves, size_t lds, int per_cu, uint64_t searchers,
                   hipStream_t stream) {
  ix->last_grid = static_cast<uint32_t>(grid);
  ix->last_waves = static_cast<uint32_t>(wg_waves);
  ix->last_lds = static_cast<uint32_t>(lds);
  ix->last_hash_log2 = p.hash_log2;
  ix->last_compact = p.vis_rbits != alaya_amd::kVisWide ? 1u : 0u;
  ix->last_per_cu = static_cast<uint32_t>(per_cu);
  ix->last_scout = p.scout;
  ix->last_scout_policy = p.scout_policy;
  ix->scout_stats_slots = p.scout ? searchers : 0;
  ix->help_stats_slots = p.help ? searchers : 0;
  ix->screen_stats_slots = p.screen ? searchers : 0;
  ix->work.reserve(4);
  p.work_counter = ix->work.as<uint32_t>();
  hip_check(hipMemsetAsync(p.work_counter, 0, 4, stream), "hipMemsetAsync");
}

void do_search(alaya_index *ix, const float *d_q, uint64_t nq, uint32_t k, uint32_t ef,
               uint32_t *d_ids, float *d_dists, uint32_t *d_cnt, hipStream_t stream,
               uint64_t *d_stamps = nullptr, bool sq8 = false, uint32_t fill_id = 0) {
  if (!ix->base.ptr) throw ArgError("index has no base vectors");
  if (!ix->has_graph) throw ArgError("index has no graph");
  if (ef == 0) throw ArgError("ef must be >= 1");
  if (k == 0 || nq == 0) return;
  if (ix->graph_n > ix->n) throw ArgError("graph has more nodes than base vectors");
  SearchParams p = graph_search_params(ix, d_q, nq, k, ef, d_ids, d_dists, d_cnt);
  p.stamps = d_stamps;
  p.fill_id = fill_id;
  if (sq8 && !ix->has_sq8) throw ArgError("index has no SQ8 codes");
  set_search_space(ix, p, sq8, ef);
  if (const char *e = std::getenv("ALAYA_HELP_FLAGS")) p.help_flags = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
  const SearchPlan plan = plan_search(ix, p, search_request(ix, p, nq, ef, stream), nq, ef, stream);
  if (p.screen >= 2) {  // 2 and 3 read the same records
    p.screen_u8 = ix->screen_copy[1].rows.as<uint8_t>();
  } else if (p.screen) {
    p.screen_rows = ix->screen_copy[0].rows.as<uint16_t>();
    p.screen_err = ix->screen_copy[0].err.as<float>();
  }
  scratch_acquire(ix, stream);
  const uint64_t searchers = static_cast<uint64_t>(plan.grid) * plan.W;
  prepare_spill(ix, p, searchers, stream);
  const int wg_waves = p.scout ? 2 * plan.W : plan.W;  // a scout wave beside every searcher
  if (p.scout) {
    ix->scout_stats.reserve(searchers * 16);
    p.scout_stats = ix->scout_stats.as<uint32_t>();
    ix->scout_policy_stats.reserve(searchers * 12);
    p.scout_policy_stats = ix->scout_policy_stats.as<uint32_t>();
  }
  if (p.help) {
    ix->help_stats.reserve(searchers * 12);
    p.help_stats = ix->help_stats.as<uint32_t>();
  }
  if (p.screen) {
    ix->screen_stats.reserve(searchers * 8);
    p.screen_stats = ix->screen_stats.as<uint32_t>();
  }
  record_launch(ix, p, plan.grid, wg_waves, plan.lds, plan.per_cu, searchers, stream);
  hip_check(alaya_amd::launch_search(*plan.variant, p, plan.grid, wg_waves, plan.lds, stream), "search launch");
  scratch_release(ix, stream);
}

// Filtered graph search (alaya_index_filtered_search*, filtered_search_kernel): planned as the plain
// (mode 0) search of the shape -- one searcher per wave, no helpers, screen, scout or two-waves mode --
// with a result pool of k entries at the end of every wave's LDS region and the occupancy of the
// filtered kernel itself.  d_allow: n_masks x ceil(n / 32) words; d_mask_of_query: nq indices or null.
//
// sq8: the search stage of the filtered SQ8 search (alaya_index_filtered_search_sq8*, filtered_sq8_search_kernel) --
// the same plan for the mode-0 SQ8 request of the shape (four waves per workgroup beside the shared scale / min,
// the spill-table second level where spill_table_log2 gives one); k is then the candidate pool's capacity m
// and d_ids / d_dists receive the nq x m candidates by code distance, for the rerank.
//
// hop: the through search (alaya_index_filtered_search_hop*, filtered_hop_search_kernel; f32 rows only) -- the same
// plan with that kernel's occupancy; d_through (nullable) receives the rows stepped through per query.
//
// range: the search stage of the range search (alaya_index_range_search*, range_search_kernel; f32 rows only) -- the
// same plan without a result pool (k = 0, d_ids / d_dists unused) and with that kernel's occupancy; d_allow may be
// null (no mask).  The kernel fills range->counts and the append buffers; the caller launches the sort.  more: the
// radius mode (alaya_index_range_search_radius*, range_more_search_kernel) -- the same plan with that kernel's occupancy.
// range with sq8: the search stage of the range search of SQ8 codes (alaya_index_range_search_sq8*,
// range_sq8_search_kernel) -- the plain mode-0 SQ8 plan of the shape, as the sq8 case, without a result pool and with
// that kernel's occupancy; range->radii are the code radii and range->counts receives the candidate counts.
void do_filtered_search(alaya_index *ix, const float *d_q, uint64_t nq, uint32_t k, uint32_t ef, const uint32_t *d_allow,
                        const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists, uint32_t *d_cnt,
                        hipStream_t stream, bool sq8 = false, bool hop = false, uint32_t *d_through = nullptr,
                        const alaya_amd::RangeParams *range = nullptr, const alaya_amd::RangeMoreParams *more = nullptr) {
  using namespace alaya_amd;
  if (range && !sq8 && ix->has_sq8)
    throw ArgError("range search of an SQ8 index: alaya_index_range_search searches f32 rows only");
  if (hop && (sq8 || ix->has_sq8))
    throw ArgError("through search of an SQ8 index: alaya_index_filtered_search_hop searches f32 rows only");
  if (!ix->base.ptr) throw ArgError("index has no base vectors");
  if (!ix->has_graph) throw ArgError("index has no graph");
  if (sq8 && !ix->has_sq8) throw ArgError("index has no SQ8 codes");
  if (!sq8 && ix->has_sq8)
    throw ArgError("filtered search of an SQ8 index: use alaya_index_filtered_search_sq8 (this call searches f32 rows only)");
  if (ef == 0) throw ArgError("ef must be >= 1");
  if (!range && (k == 0 || k > 224)) throw ArgError("filtered search: k must be in 1..224");
  if (nq == 0) return;
  if (ix->graph_n > ix->n) throw ArgError("graph has more nodes than base vectors");
  SearchParams p = graph_search_params(ix, d_q, nq, k, ef, d_ids, d_dists, d_cnt);
  p.fill_id = 0xffffffffu;  // empty result slots: (all-ones id, FLT_MAX), exact_search's convention
  set_search_space(ix, p, sq8, ef);  // (f32 rows: the bitset, as do_search plans it)
  const SearchVariant &plain = resolve_search_variant({ix->dim, p.ip, p.sq8_order, ix->generic, 0});
  int W = search_waves(p);
  while (W > 1 && static_cast<uint64_t>(W) > nq) W /= 2;
  p.hash_log2 = size_visited(ix, p, plain, nq, ef, W, k, hop, range != nullptr, more != nullptr);
  const size_t traversal_lds = search_wave_lds_bytes(ix->stride, ef, p.hash_log2, p.vis_rbits != kVisWide, p.sq8_order);
  p.wave_lds = static_cast<uint32_t>(traversal_lds + (range ? 0 : filter_result_lds_bytes(k)));
  FilterParams f{};
  f.allow = d_allow;
  f.mask_of_query = d_mask_of_query;
  f.mask_words = static_cast<uint32_t>((ix->n + 31) / 32);
  f.k = k;
  f.result_off = static_cast<uint32_t>(traversal_lds);
  const size_t lds = search_shared_lds_bytes(ix->stride, sq8) + static_cast<size_t>(W) * p.wave_lds;
  if (lds > kLdsPerCu)
    throw ArgError(range ? "range search: ef / dim too large for the LDS budget"
                         : "filtered search: k / ef / dim too large for the LDS budget");
  int per_cu = 0;
  hip_check(more    ? range_more_search_occupancy(ix->dim, ix->generic, p.ip, W, lds, &per_cu)
            : range && sq8 ? range_sq8_search_occupancy(ix->dim, p.sq8_order, p.ip, W, lds, &per_cu)
            : range ? range_search_occupancy(ix->dim, ix->generic, p.ip, W, lds, &per_cu)
            : sq8 ? filtered_sq8_search_occupancy(ix->dim, p.sq8_order, p.ip, W, lds, &per_cu)
            : hop ? filtered_hop_search_occupancy(ix->dim, ix->generic, p.ip, W, lds, &per_cu)
                : filtered_search_occupancy(ix->dim, ix->generic, p.ip, W, lds, &per_cu),
            "occupancy");
  per_cu = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(per_cu, max_search_waves_per_cu() / W)));
  const uint64_t cus = static_cast<uint64_t>(stream_cus(ix, stream));
  int grid = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>((nq + W - 1) / W, static_cast<uint64_t>(per_cu) * cus)));
  // diagnostics (ALAYA_FILTER_GRID, include/alaya_hip.h): fewer workgroups than queries, so every wave runs
  // several queries of the launch, one after the other, on one result pool
  if (const char *e = std::getenv("ALAYA_FILTER_GRID")) grid = std::max(1, std::min(grid, std::atoi(e)));
  scratch_acquire(ix, stream);
  const uint64_t searchers = static_cast<uint64_t>(grid) * W;
  prepare_spill(ix, p, searchers, stream);
  record_launch(ix, p, grid, W, lds, per_cu, searchers, stream);  // (no scout, helpers or screen: p has none set)
  hip_check(more    ? launch_range_more_search(p, f, *range, *more, grid, W, lds, stream)
            : range && sq8 ? launch_range_sq8_search(p, f, *range, grid, W, lds, stream)
            : range ? launch_range_search(p, f, *range, grid, W, lds, stream)
            : sq8 ? launch_filtered_sq8_search(p, f, grid, W, lds, stream)
            : hop ? launch_filtered_hop_search(p, f, HopParams{d_through}, grid, W, lds, stream)
                  : launch_filtered_search(p, f, grid, W, lds, stream),
            "filtered search launch");
  scratch_release(ix, stream);
}

// Default of ALAYA_SEARCH_SCREEN per kernel width: on where the screened search measured faster on
// MI355X against the plain kernel (GIST-shaped 1k queries, d = 512 +7 %,
// 768 +12 %, 960 +29 %, 1024 +27 %; the two-waves-per-SIMD batches +18 % / +41 %) -- every width
// that has a screening kernel.
// The format (SearchParams::screen: 1 = f16, 2 = 8-bit records in f32 arithmetic, 3 = the same records
// under integer dot products) is the one that measured fastest for the width.  Round 8: the records
// against the f16 copy d = 768 +16 %, 960 +11 %, 1024 +16 %, d = 512 equal.  Round 10 (DESIGN.md
// section 3, profiles/r10/shapes_ab.jsonl): the integer pass against the width's previous default
// d = 512 +13 %, 768 +8 %, 960 +18 %, 1024 +16 %, the two-waves-per-SIMD batches +15 % / +22 % -- every
// screened width.  ALAYA_SEARCH_SCREEN = 8 / 1 still ask for the other two.
uint32_t screen_default(uint32_t dim) {
  return (dim == 512 || dim == 768 || dim == 960 || dim == 1024) ? 3u : 0u;
}

// Rows [first, first + count) of the base into the screening copy of `format`.
void screen_fill(alaya_index *ix, uint32_t format, uint64_t first, uint64_t count, hipStream_t stream) {
  alaya_index::ScreenCopy &c = ix->screen_copy[format - 1];
  hip_check(format == 2 ? alaya_amd::launch_screen_rows_u8(ix->base.as<float>(), first, count, ix->stride,
                                                           c.rows.as<uint8_t>(), stream)
                        : alaya_amd::launch_screen_rows(ix->base.as<float>(), first, count, ix->stride,
                                                        c.rows.as<uint16_t>(), c.err.as<float>(), stream),
            "screening copy");
}

// Whether this launch screens, and on which copy: the shape has a screening kernel,
// ALAYA_SEARCH_SCREEN (0 = off, 8 = the 8-bit records in f32 arithmetic, 9 = the same records under
// integer dot products with the query's own codes, anything else = f16; read per launch; unset =
// screen_default) names a format, and that format's copy exists or can be built now, on the search's
// stream.  Sets ix->screen_format.  An allocation failure is not an error: the search runs the plain
// kernel.
bool ensure_screen(alaya_index *ix, const SearchParams &p, bool eligible, hipStream_t stream) {
  ix->screen_format = 0;
  if (!eligible || !alaya_amd::search_has_screen(ix->dim, p.sq8_order, ix->generic, p.ip)) return false;
  const char *e = std::getenv("ALAYA_SEARCH_SCREEN");
  const int asked = e && e[0] ? std::atoi(e) : -1;
  const uint32_t format =
      asked < 0 ? screen_default(ix->dim) : (asked == 0 ? 0u : (asked == 9 ? 3u : (asked == 8 ? 2u : 1u)));
  if (format == 0) return false;
  const uint32_t copy = format == 3 ? 2u : format;  // the integer pass reads format 2's records
  alaya_index::ScreenCopy &c = ix->screen_copy[copy - 1];
  if (c.failed) return false;
  if (!c.ready) {
    const uint64_t rows = std::max<uint64_t>(std::max(ix->capacity, ix->n), 1);
    try {
      if (rows > c.cap) {
        c.rows.release();
        c.err.release();
        c.cap = 0;
        if (copy == 2) {
          c.rows.reserve(rows * alaya_amd::screen_u8_record_bytes(ix->stride));
        } else {
          c.rows.reserve(rows * ix->stride * 2);
          c.err.reserve(rows * 4);
        }
        c.cap = rows;
      }
    } catch (const DeviceError &) {
      (void)hipGetLastError();
      c.rows.release();
      c.err.release();
      c.cap = 0;
      c.failed = true;
      return false;
    }
    scratch_acquire(ix, stream);  // after every earlier launch that may still read the buffers
    screen_fill(ix, copy, 0, ix->n, stream);
    c.ready = true;
  }
  ix->screen_format = format;
  return true;
}

// The base is gone or replaced: nothing keeps its screening copies alive.
void screen_drop(alaya_index *ix) {
  for (alaya_index::ScreenCopy &c : ix->screen_copy) {
    c.rows.release();
    c.err.release();
    c.cap = 0;
    c.ready = false;
    c.failed = false;
  }
  ix->screen_format = 0;
  ix->screen_stats_slots = 0;
}

void ensure_norms(alaya_index *ix, hipStream_t stream) {
  if (ix->norms_ready) return;
  ix->norms.reserve(std::max<uint64_t>(ix->n, 1) * 4);
  hip_check(alaya_amd::launch_row_norms(ix->base.as<float>(), ix->n, ix->stride, ix->norms.as<float>(), stream),
            "row norms");
  std::vector<float> h(ix->n);
  hip_check(hipMemcpyAsync(h.data(), ix->norms.ptr, ix->n * 4, hipMemcpyDeviceToHost, stream), "D2H");
  hip_check(hipStreamSynchronize(stream), "norms");
  float mx = 0.f;
  for (float v : h) mx = std::max(mx, v);
  ix->max_norm = std::sqrt(mx) * 1.0001f;
  if (ix->metric != ALAYA_METRIC_L2) {
    // inner products rank by the contraction alone: the scans read zeros where L2 reads |b|^2
    ix->flat_bias.reserve(std::max<uint64_t>(ix->n, 1) * 4);
    hip_check(hipMemsetAsync(ix->flat_bias.ptr, 0, std::max<uint64_t>(ix->n, 1) * 4, stream), "flat bias");
  }
  ix->norms_ready = true;
}

// Base chunks per query group: enough blocks to cover the CUs, each chunk >= 64 rows.
int flat_chunks(alaya_index *ix, int nqg, uint64_t rows) {
  int chunks = (ix->num_cus + nqg - 1) / nqg;
  chunks = std::max(8, (chunks + 7) / 8 * 8);
  const uint64_t max_chunks = std::max<uint64_t>(8, (rows / 64) / 8 * 8);
  return static_cast<int>(std::min<uint64_t>(chunks, max_chunks));
}

// Chunks per query group of the single-role f16 scan (256 queries per block, one block per CU): the
// fewest chunks that give every CU a block; past that, the chunk count in 8..64 whose blocks fill
// whole rounds of the CUs best (fewer chunks on ties -- each chunk adds ~32 ln(rows) appends per
// query).  Every chunk keeps >= 4 records.
int flat_tiles_chunks(alaya_index *ix, uint64_t nq, uint64_t scan_tiles) {
  const uint64_t qpb = alaya_amd::flat_tiles_queries();
  const uint64_t nqg = (nq + qpb - 1) / qpb;
  const uint64_t cus = static_cast<uint64_t>(std::max(1, ix->num_cus));
  const uint64_t cap = std::max<uint64_t>(8, std::min<uint64_t>(256, (scan_tiles / 4) / 8 * 8));
  if (nqg * 8 < cus) return static_cast<int>(std::min<uint64_t>(cap, (cus + nqg - 1) / nqg + 7) / 8 * 8);
  uint64_t best = 8;
  double best_eff = 0.0;
  for (uint64_t c = 8; c <= std::min<uint64_t>(64, cap); c += 8) {
    const uint64_t b = nqg * c;
    const double eff = static_cast<double>(b) / static_cast<double>((b + cus - 1) / cus * cus);
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = c;
    }
  }
  return static_cast<int>(best);
}

// the flat scans' per-row bias: |b|^2 for L2, zeros for IP / COS
const float *flat_bias(const alaya_index *ix) {
  return ix->metric == ALAYA_METRIC_L2 ? ix->norms.as<float>() : ix->flat_bias.as<float>();
}

void ensure_tiles(alaya_index *ix, int base_exp, hipStream_t stream) {
  // records built for another metric carry the wrong bias: never reused (set_base also drops them)
  if (ix->tiles_ready && ix->tiles_exp == base_exp && ix->tiles_metric == ix->metric) return;
  const size_t bytes = alaya_amd::flat_tiles_bytes(ix->stride, ix->n);
  ix->flat_tiles.reserve(std::max<size_t>(bytes, 256));
  hip_check(alaya_amd::launch_flat_tiles(ix->base.as<float>(), ix->n, ix->stride, flat_bias(ix),
                                         ix->has_valid ? ix->valid.as<uint32_t>() : nullptr, base_exp,
                                         ix->flat_tiles.as<unsigned char>(), stream),
            "flat tile records");
  ix->tiles_ready = true;
  ix->tiles_exp = base_exp;
  ix->tiles_metric = ix->metric;
}

// Prescan: the same scan over rows 0, S, 2S, ... (S = ALAYA_FLAT_PRESCAN; default 0 = off: on
// config 2 it cuts fold rounds 846 -> 302 per block but costs more than it saves),
// then per query the sample's 32nd-best approximate distance as every chunk's starting threshold.
// The sample's 32nd is about the whole base's (32 S)-th, so the full scan appends ~S candidates
// per (query, chunk) instead of ~32 (1 + ln(chunk rows / 32)).  Results are unchanged: the
// threshold only rejects rows that cannot reach the merged 32, and the merge's bound uses it.
void flat_prescan(alaya_index *ix, alaya_amd::FlatParams &p, hipStream_t s) {
  const char *env = std::getenv("ALAYA_FLAT_PRESCAN");
  const uint64_t step = env ? std::strtoull(env, nullptr, 10) : 0;
  // the scan of the sample `q` describes, over nqg query groups, then the thresholds, which p starts from
  auto sample_scan = [&](alaya_amd::FlatParams q, int nqg) {
    q.tau_init = nullptr;
    q.out_ids = nullptr;
    q.out_dists = nullptr;
    q.flags = nullptr;
    q.merge_count = nullptr;
    q.ablate = 0;
    ix->flat_tau.reserve(p.nq * 4);
    q.tau_out = ix->flat_tau.as<float>();
    hip_check(alaya_amd::launch_flat_scan(q, nqg * q.n_chunks, s), "flat prescan");
    hip_check(alaya_amd::launch_flat_threshold(q, s), "flat threshold");
    p.tau_init = q.tau_out;
  };
  if (p.tiles != nullptr) {
    // The single-role scan's prescan: group minima over a sample of whole tile records (every S-th;
    // default S = records / 4096, on when the base has >= 8192 records, ALAYA_FLAT_PRESCAN=S forces S,
    // 1 turns it off), one block per (query group, group of sampled records); the 32nd smallest
    // of a query's group minima is its starting threshold (flat_group_threshold_kernel).
    const uint64_t nt = p.n_scan_tiles;
    const char *genv = std::getenv("ALAYA_FLAT_PRESCAN_GROUPS");  // diagnostics: groups (default 64)
    const char *senv = std::getenv("ALAYA_FLAT_PRESCAN_SAMPLE");  // diagnostics: sampled records (4096)
    const uint64_t want_sample = senv ? std::max<uint64_t>(32, std::strtoull(senv, nullptr, 10)) : 4096;
    uint64_t S = env ? step : (nt >= 2 * want_sample ? nt / want_sample : 0);
    if (S < 1 || (env && S < 2)) return;
    const uint64_t sample = (nt + S - 1) / S;
    // groups of >= 1 sampled record (64+ at the defaults); the minima (groups x nq floats) fit the
    // candidate buffers (n_chunks >= 8 lists of 32 per query)
    const uint64_t want_groups = genv ? std::strtoull(genv, nullptr, 10) : 64;
    const uint64_t groups = std::min<uint64_t>(std::min<uint64_t>(256, want_groups), sample) / 8 * 8;
    if (groups < static_cast<uint64_t>(alaya_amd::flat_shortlist())) return;
    alaya_amd::FlatParams q = p;
    q.tile_step = static_cast<uint32_t>(S);
    q.n_scan_tiles = sample;
    q.n_chunks = static_cast<int>(groups);
    const int qpb = alaya_amd::flat_tiles_queries();
    sample_scan(q, static_cast<int>((p.nq + qpb - 1) / qpb));
    return;
  }
  if (step < 2 || p.n / step < 1024) return;
  // the slabbed wide scan (rows past 224 floats) reads contiguous rows and has no row_step: its
  // "sample" would be the first n/S rows, so the prescan is off there
  if (alaya_amd::flat_query_width(ix->stride) != 0) return;
  alaya_amd::FlatParams q = p;
  q.n = (p.n + step - 1) / step;
  q.row_step = static_cast<uint32_t>(step);
  const int nqg = static_cast<int>((p.nq + 127) / 128);
  q.n_chunks = flat_chunks(ix, nqg, q.n);  // <= p.n_chunks: the candidate buffers fit
  sample_scan(q, nqg);
}

alaya_amd::FlatParams flat_params(alaya_index *ix, const float *d_q, uint64_t nq, uint32_t k, uint32_t *d_ids,
                                  float *d_dists, uint32_t *d_flags, int *blocks, hipStream_t stream,
                                  bool no_single = false) {
  if (!ix->base.ptr) throw ArgError("index has no base vectors");
  if (ix->metric != ALAYA_METRIC_L2 && ix->metric != ALAYA_METRIC_IP && ix->metric != ALAYA_METRIC_COS)
    throw ArgError("the flat MFMA path supports the L2, IP and COS metrics");
  if (ix->generic) throw ArgError("the flat MFMA path ranks float32 rows (not the generic non-float order)");
  if (alaya_amd::flat_scan_lds(ix->stride) == 0) throw ArgError("no flat MFMA scan for this row stride");
  if (k == 0 || k > static_cast<uint32_t>(alaya_amd::flat_max_k()))
    throw ArgError("flat search needs 1 <= k <= " + std::to_string(alaya_amd::flat_max_k()));
  alaya_amd::FlatParams p{};
  p.base = ix->base.as<float>();
  p.n = ix->n;
  p.dim = ix->dim;
  p.stride = ix->stride;
  p.norms = flat_bias(ix);
  p.ip = ix->metric != ALAYA_METRIC_L2;
  p.valid = ix->has_valid ? ix->valid.as<uint32_t>() : nullptr;
  p.max_norm = ix->max_norm;
  // The contraction that ranks the shortlist (all three feed the same exact rescoring and proof):
  //  * single-pass f16 (default for rows of <= 224 floats, the warp-specialised scan): one MFMA per
  //    16 k on power-of-two-scaled operands; needs the row scale 2^s in range (|s| <= 60);
  //  * bf16 hi/lo split (wide rows, or rows out of the f16 scale's range, or
  //    ALAYA_FLAT_CONTRACTION=bf16x3), unless the rows are large enough for bf16(x) to overflow;
  //  * f32 MFMA (ALAYA_FLAT_CONTRACTION=f32 or ALAYA_FLAT_F32).
  const char *fc = std::getenv("ALAYA_FLAT_CONTRACTION");
  const std::string want = fc ? fc : (std::getenv("ALAYA_FLAT_F32") ? "f32" : "auto");
  if (want != "auto" && want != "f16" && want != "bf16x3" && want != "f32")
    throw ArgError("ALAYA_FLAT_CONTRACTION must be f16, bf16x3 or f32");
  p.base_exp = alaya_amd::flat_base_exp(ix->max_norm);
  const bool narrow = alaya_amd::flat_query_width(ix->stride) == 0;
  p.single = !no_single && (want == "auto" || want == "f16") && narrow && alaya_amd::flat_ws_available(0) &&
             std::abs(p.base_exp) <= 60 && ix->max_norm > 0.f && std::isfinite(ix->max_norm);
  p.split = !p.single && want != "f32" && ix->max_norm < 1e18f;
  ix->flat_contraction = p.single ? 2 : (p.split ? 1 : 0);
  p.queries = d_q;
  p.nq = nq;
  p.q_stride = ix->dim;
  p.k_acc = ix->stride;
  if (const uint32_t width = alaya_amd::flat_query_width(ix->stride)) {
    // wide rows: the scan reads the queries as zero-padded rows of the slabbed width
    ix->flat_q.reserve(nq * width * 4);
    hip_check(alaya_amd::launch_pad_queries(d_q, nq, ix->dim, width, ix->flat_q.as<float>(), stream), "pad queries");
    p.queries = ix->flat_q.as<float>();
    p.q_stride = width;
    p.k_acc = width;
  }
  // the single pass runs the single-role scan over the cached tile records (ALAYA_FLAT_TILES=0 keeps
  // the warp-specialised scan, which converts the f32 rows itself)
  const char *tenv = std::getenv("ALAYA_FLAT_TILES");
  const bool tiles = p.single && !(tenv && tenv[0] == '0') && alaya_amd::flat_tiles_bytes(ix->stride, ix->n) > 0;
  int nqg = 0, chunks = 0;
  if (tiles) {
    ensure_tiles(ix, p.base_exp, stream);
    p.tiles = ix->flat_tiles.as<unsigned char>();
    p.n_scan_tiles = (ix->n + 31) / 32;
    p.tile_step = 1;
    const int qpb = alaya_amd::flat_tiles_queries();
    nqg = static_cast<int>((nq + qpb - 1) / qpb);
    chunks = flat_tiles_chunks(ix, nq, p.n_scan_tiles);
    ix->tiles_cand.reserve(static_cast<size_t>(nqg) * chunks * qpb * alaya_amd::flat_tiles_buf() * 8);
    p.tiles_buf = ix->tiles_cand.as<uint64_t>();
    ix->tiles_qexp.reserve(nq * 4);
    p.tiles_qexp = ix->tiles_qexp.as<int>();
  } else {
    nqg = static_cast<int>((nq + 127) / 128);
    chunks = flat_chunks(ix, nqg, ix->n);
  }
  p.n_chunks = chunks;
  p.row_step = 1;
  const char *spin = std::getenv("ALAYA_FLAT_SPIN_LIMIT");  // debug override (tests force an abort)
  p.spin_limit = spin ? static_cast<uint32_t>(std::strtoul(spin, nullptr, 10)) : (1u << 20);
  const size_t cand = static_cast<size_t>(chunks) * nq * alaya_amd::flat_shortlist();
  ix->cand_d.reserve(cand * 4);
  ix->cand_i.reserve(cand * 4);
  p.cand_d = ix->cand_d.as<float>();
  p.cand_i = ix->cand_i.as<uint32_t>();
  p.k = k;
  p.out_ids = d_ids;
  p.out_dists = d_dists;
  p.flags = d_flags;
  *blocks = nqg * chunks;
  return p;
}

// One flat search on device buffers: row norms (first call only), the launch's parameters, the optional
// prescan, the scan and the merge.  Returns the parameters (the host entry point reads p.single).
alaya_amd::FlatParams flat_scan_merge(alaya_index *ix, const float *d_q, uint64_t nq, uint32_t k, uint32_t *d_ids,
                                      float *d_dists, uint32_t *d_flags, hipStream_t s, bool no_single = false) {
  ensure_norms(ix, s);
  int blocks = 0;
  alaya_amd::FlatParams p = flat_params(ix, d_q, nq, k, d_ids, d_dists, d_flags, &blocks, s, no_single);
  flat_prescan(ix, p, s);
  hip_check(alaya_amd::launch_flat_scan(p, blocks, s), "flat scan");
  hip_check(alaya_amd::launch_flat_merge(p, s), "flat merge");
  return p;
}

// The rerank of an SQ8 search: rescores on the f32 rows, against d_q, the ids the search stage left in
// ix->sq_ids (r.n_src per query) and writes the first r.k to d_ids / d_dists.  The caller sets r.k, r.n_src,
// r.n_take, r.zeros and r.fill_id.
void rerank_sq_ids(alaya_index *ix, const float *d_q, uint64_t nq, alaya_amd::RerankParams r, uint32_t *d_ids,
                   float *d_dists, hipStream_t s) {
  SearchParams p = base_params(ix);
  p.queries = d_q;
  p.nq = nq;
  p.q_stride = ix->dim;
  r.search_ids = ix->sq_ids.as<uint32_t>();
  r.out_ids = d_ids;
  r.out_dists = d_dists;
  hip_check(alaya_amd::launch_rerank(p, r, s), "rerank launch");
  scratch_release(ix, s);  // the rerank read the search's ids from the index's sq_ids buffer
}

// ---- what the filtered entry points check of their masks ------------------------------------------
// what: the message's prefix, "filtered search" or "flat filtered search".
void check_mask_indices(const char *what, const uint32_t *h_mask_of_query, uint64_t nq, uint32_t n_masks) {
  for (uint64_t i = 0; i < nq; ++i)
    if (h_mask_of_query[i] >= n_masks) throw ArgError(std::string(what) + ": mask_of_query holds an index past n_masks");
}
// host_indices: mask_of_query can be read here (the host entry points'); a device pointer is taken as it is.
void check_masks(const char *what, uint64_t nq, uint32_t n_masks, const uint32_t *mask_of_query, bool host_indices) {
  if (nq && (n_masks == 0 || (n_masks > 1 && !mask_of_query)))
    throw ArgError(std::string(what) + ": mask_of_query may be null only with one mask");
  if (host_indices && mask_of_query) check_mask_indices(what, mask_of_query, nq, n_masks);
}

// ---- staging of the host entry points: the index's own buffers, on ix->stream ----------------------
// `what` labels a failed copy; the entry points' labels differ and are part of their error texts.
const float *stage_rows(alaya_index *ix, DevBuf &buf, const float *rows, uint64_t nq, const char *what) {
  buf.reserve(nq * ix->dim * 4);
  hip_check(hipMemcpyAsync(buf.ptr, rows, nq * ix->dim * 4, hipMemcpyHostToDevice, ix->stream), what);
  return buf.as<float>();
}
// Reserves the query buffer and the (nq, k) result buffers the call uses, then uploads the queries.
const float *stage_queries(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                           const char *what = "upload queries", bool dists = true, bool counters = true) {
  ix->q_buf.reserve(nq * ix->dim * 4);
  ix->id_buf.reserve(nq * k * 4);
  if (dists) ix->dist_buf.reserve(nq * k * 4);
  if (counters) ix->cnt_buf.reserve(nq * 16);
  return stage_rows(ix, ix->q_buf, queries, nq, what);
}
// The SQ8 rerank's own query form: uploaded only when given and not the queries themselves, else null.
const float *stage_rerank_queries(alaya_index *ix, const float *rerank_queries, const float *queries, uint64_t nq,
                                  const char *what = "upload rerank queries") {
  if (!rerank_queries || rerank_queries == queries) return nullptr;
  return stage_rows(ix, ix->rr_q_buf, rerank_queries, nq, what);
}
const uint32_t *stage_masks(alaya_index *ix, const uint32_t *allow_words, uint32_t n_masks) {
  const size_t bytes = static_cast<size_t>(n_masks) * ((ix->n + 31) / 32) * 4;
  ix->allow_buf.reserve(bytes);
  hip_check(hipMemcpyAsync(ix->allow_buf.ptr, allow_words, bytes, hipMemcpyHostToDevice, ix->stream), "upload masks");
  return ix->allow_buf.as<uint32_t>();
}
// group_buf is reserved for nq indices even when none are given (null then, as the kernels expect)
const uint32_t *stage_mask_indices(alaya_index *ix, const uint32_t *mask_of_query, uint64_t nq) {
  ix->group_buf.reserve(nq * 4);
  if (!mask_of_query) return nullptr;
  hip_check(hipMemcpyAsync(ix->group_buf.ptr, mask_of_query, nq * 4, hipMemcpyHostToDevice, ix->stream),
            "upload mask indices");
  return ix->group_buf.as<uint32_t>();
}
// ids, and dists / counters where asked for, back to the host; the caller synchronises (stream_sync)
void fetch_results(alaya_index *ix, uint64_t nq, uint32_t k, uint32_t *ids, float *dists, uint32_t *counters) {
  hip_check(hipMemcpyAsync(ids, ix->id_buf.ptr, nq * k * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
  if (dists) hip_check(hipMemcpyAsync(dists, ix->dist_buf.ptr, nq * k * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
  if (counters)
    hip_check(hipMemcpyAsync(counters, ix->cnt_buf.ptr, nq * 16, hipMemcpyDeviceToHost, ix->stream), "D2H");
}
void stream_sync(alaya_index *ix, const char *what) { hip_check(hipStreamSynchronize(ix->stream), what); }

}  // namespace

extern "C" {

const char *alaya_last_error(void) { return g_last_error.c_str(); }

#ifndef ALAYA_BUILD_INFO
#define ALAYA_BUILD_INFO "source=unknown"
#endif
const char *alaya_build_info(void) { return ALAYA_BUILD_INFO; }

int alaya_device_count(int *count) {
  return guarded([&] {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
  });
}

// ---- graphs ---------------------------------------------------------------------------------
int alaya_hbm_stream_read(int device, uint64_t bytes, int iters, double *gbs) {
  return guarded([&] {
    if (!gbs || bytes < (1u << 20) || iters < 1) throw ArgError("invalid arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) throw DeviceError("no HIP device available");
    if (device < 0 || device >= count) throw ArgError("device ordinal out of range");
    hip_check(hipSetDevice(device), "hipSetDevice");
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
    bytes = bytes / 16 * 16;
    DevBuf buf, sink;
    buf.reserve(bytes);
    sink.reserve(4);
    hipStream_t s = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    hip_check(hipEventCreate(&a), "hipEventCreate");
    hip_check(hipEventCreate(&b), "hipEventCreate");
    double best = 0.0;
    try {
      hip_check(hipMemsetAsync(buf.ptr, 0, bytes, s), "memset");
      for (int shape = 0; shape < 3; ++shape) {
        for (int occ : {8, 16}) {  // 256-thread workgroups per CU
          const int grid = prop.multiProcessorCount * occ;
          hip_check(alaya_amd::launch_stream_read(buf.ptr, bytes, grid, shape, sink.as<float>(), s), "stream read");
          for (int it = 0; it < iters; ++it) {
            hip_check(hipEventRecord(a, s), "hipEventRecord");
            hip_check(alaya_amd::launch_stream_read(buf.ptr, bytes, grid, shape, sink.as<float>(), s), "stream read");
            hip_check(hipEventRecord(b, s), "hipEventRecord");
            hip_check(hipEventSynchronize(b), "hipEventSynchronize");
            float ms = 0.f;
            hip_check(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime");
            best = std::max(best, static_cast<double>(bytes) / (ms * 1e6));
          }
        }
      }
    } catch (...) {
      (void)hipStreamSynchronize(s);
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
      (void)hipStreamDestroy(s);
      throw;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    (void)hipStreamDestroy(s);
    *gbs = best;
  });
}

int alaya_graph_build_hnsw(const float *data, uint64_t n, uint32_t dim, int metric, uint32_t R,
                           uint32_t ef_construction, uint32_t num_threads, uint64_t seed,
                           alaya_graph **out) {
  return guarded([&] {
    if (!out || (n && !data) || dim == 0) throw ArgError("invalid arguments");
    if ((metric & ~ALAYA_DIST_GENERIC) < ALAYA_METRIC_L2 || (metric & ~ALAYA_DIST_GENERIC) > ALAYA_METRIC_COS)
      throw ArgError("unknown metric");
    if (n >= (1ull << 31)) throw ArgError("ids must stay below 2^31 (LinearPool checked bit)");
    auto g = std::make_unique<alaya_graph>();
    g->g = alaya_amd::build_hnsw(data, n, dim, metric, R, ef_construction, num_threads, seed);
    *out = g.release();
  });
}

int alaya_graph_load(const char *path, int id_bytes, alaya_graph **out) {
  return guarded([&] {
    if (!out || !path) throw ArgError("invalid arguments");
    auto g = std::make_unique<alaya_graph>();
    g->g = alaya_amd::load_graph(path, id_bytes);
    *out = g.release();
  });
}

int alaya_graph_save(const alaya_graph *g, const char *path, int id_bytes, uint64_t capacity,
                     const uint8_t *valid_bitmap) {
  return guarded([&] {
    if (!g || !path) throw ArgError("invalid arguments");
    alaya_amd::save_graph(g->g, path, id_bytes, capacity, valid_bitmap);
  });
}

int alaya_graph_info(const alaya_graph *g, uint64_t *n, uint32_t *R, int *has_overlay,
                     uint32_t *upper_R, uint32_t *ep, uint32_t *max_level,
                     uint64_t *n_upper_edges, uint32_t *n_eps) {
  return guarded([&] {
    if (!g) throw ArgError("null graph");
    if (n) *n = g->g.n;
    if (R) *R = g->g.R;
    if (has_overlay) *has_overlay = g->g.has_overlay ? 1 : 0;
    if (upper_R) *upper_R = g->g.upper_R;
    if (ep) *ep = g->g.ep;
    if (max_level) *max_level = g->g.max_level();
    if (n_upper_edges) *n_upper_edges = g->g.upper_edges.size();
    if (n_eps) *n_eps = static_cast<uint32_t>(g->g.eps.size());
  });
}

int alaya_graph_export(const alaya_graph *g, uint32_t *l0, uint32_t *levels, uint64_t *upper_off,
                       uint32_t *upper_edges, uint32_t *eps) {
  return guarded([&] {
    if (!g) throw ArgError("null graph");
    const HostGraph &h = g->g;
    if (l0) std::memcpy(l0, h.l0.data(), h.l0.size() * 4);
    if (levels && !h.levels.empty()) std::memcpy(levels, h.levels.data(), h.levels.size() * 4);
    if (upper_off && !h.upper_off.empty()) std::memcpy(upper_off, h.upper_off.data(), h.upper_off.size() * 8);
    if (upper_edges && !h.upper_edges.empty())
      std::memcpy(upper_edges, h.upper_edges.data(), h.upper_edges.size() * 4);
    if (eps && !h.eps.empty()) std::memcpy(eps, h.eps.data(), h.eps.size() * 4);
  });
}

int alaya_graph_import(uint64_t n, uint32_t R, const uint32_t *l0, const uint32_t *levels,
                       const uint64_t *upper_off, const uint32_t *upper_edges,
                       uint64_t n_upper_edges, uint32_t upper_R, uint32_t ep, const uint32_t *eps,
                       uint32_t n_eps, alaya_graph **out) {
  return guarded([&] {
    if (!out || (n && !l0) || R == 0 || R > 64) throw ArgError("invalid graph arrays (R must be 1..64)");
    auto g = std::make_unique<alaya_graph>();
    HostGraph &h = g->g;
    h.n = n;
    h.R = R;
    h.l0.assign(l0, l0 + n * R);
    if (levels) {
      if (!upper_off || (n_upper_edges && !upper_edges) || upper_R == 0 || upper_R > 64)
        throw ArgError("invalid overlay arrays (upper_R must be 1..64)");
      if (n && ep >= n) throw ArgError("entry point out of range");
      h.has_overlay = true;
      h.levels.assign(levels, levels + n);
      h.upper_off.assign(upper_off, upper_off + n);
      h.upper_edges.assign(upper_edges, upper_edges + n_upper_edges);
      h.upper_R = upper_R;
      h.ep = ep;
      for (uint64_t i = 0; i < n; ++i)
        if (h.levels[i] && h.upper_off[i] + static_cast<uint64_t>(h.levels[i]) * upper_R > n_upper_edges)
          throw ArgError("upper_off/levels exceed upper_edges");
    } else {
      if (n_eps == 0 && n) throw ArgError("graph without overlay needs entry points");
      h.eps.assign(eps, eps + n_eps);
    }
    *out = g.release();
  });
}

void alaya_graph_free(alaya_graph *g) { delete g; }

// ---- device index ----------------------------------------------------------------------------
int alaya_index_create(int device, alaya_index **out) {
  return guarded([&] {
    if (!out) throw ArgError("null out");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
      throw DeviceError("no HIP device available (the MI355X search path has no CPU fallback)");
    if (device < 0 || device >= count) throw ArgError("device ordinal out of range");
    auto ix = std::make_unique<alaya_index>();
    ix->device = device;
    set_device(ix.get());
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
    ix->num_cus = prop.multiProcessorCount;
    hip_check(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking), "hipStreamCreate");
    hip_check(hipEventCreateWithFlags(&ix->scratch_ev, hipEventDisableTiming), "hipEventCreate");
    *out = ix.release();
  });
}

void alaya_index_destroy(alaya_index *ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  if (ix->scratch_used) (void)hipEventSynchronize(ix->scratch_ev);
  if (ix->scratch_ev) (void)hipEventDestroy(ix->scratch_ev);
  if (ix->stream) (void)hipStreamDestroy(ix->stream);
  delete ix;
}

int alaya_index_set_base(alaya_index *ix, const float *rows, uint64_t n, uint32_t dim, int metric,
                         const uint8_t *valid_bitmap) {
  return guarded([&] {
    if (!ix || (n && !rows) || dim == 0) throw ArgError("invalid arguments");
    const bool generic = (metric & ALAYA_DIST_GENERIC) != 0;
    metric &= ~ALAYA_DIST_GENERIC;
    if (metric < ALAYA_METRIC_L2 || metric > ALAYA_METRIC_COS) throw ArgError("unknown metric");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    scratch_drain(ix);
    const uint32_t stride = round_up32(dim);
    if (ix->has_sq8) {  // new rows: the codes describe the old ones, whatever the shape
      ix->has_sq8 = false;
      ix->codes.release();
      ix->sq_min.release();
      ix->sq_max.release();
    }
    ix->base.release();
    screen_drop(ix);
    ix->base.reserve(std::max<uint64_t>(n, 1) * stride * 4);
    if (n) {
      hip_check(hipMemset2DAsync(ix->base.ptr, static_cast<size_t>(stride) * 4, 0,
                                 static_cast<size_t>(stride) * 4, n, ix->stream), "memset");
      hip_check(hipMemcpy2DAsync(ix->base.ptr, static_cast<size_t>(stride) * 4, rows,
                                 static_cast<size_t>(dim) * 4, static_cast<size_t>(dim) * 4, n,
                                 hipMemcpyHostToDevice, ix->stream), "upload base");
    }
    ix->has_valid = valid_bitmap != nullptr;
    ix->valid.release();
    if (valid_bitmap) {
      const size_t words = (n + 31) / 32;
      std::vector<uint32_t> w(std::max<size_t>(words, 1), 0);
      std::memcpy(w.data(), valid_bitmap, (n + 7) / 8);
      ix->valid.reserve(w.size() * 4);
      hip_check(hipMemcpyAsync(ix->valid.ptr, w.data(), w.size() * 4, hipMemcpyHostToDevice,
                               ix->stream), "upload bitmap");
      hip_check(hipStreamSynchronize(ix->stream), "sync");
    }
    hip_check(hipStreamSynchronize(ix->stream), "sync");
    ix->n = n;
    ix->dim = dim;
    ix->stride = stride;
    ix->metric = metric;
    ix->generic = generic;
    ix->overflow.release();
    ix->overflow_clean = 0;
    ix->norms_ready = false;
    ix->tiles_ready = false;
    ix->capacity = n;
    ix->upd_graph.reset();
    ix->upd_rows.reset();
    ix->upd_ctx.reset();
  });
}

int alaya_index_set_graph(alaya_index *ix, const alaya_graph *g) {
  return guarded([&] {
    if (!ix || !g) throw ArgError("invalid arguments");
    const HostGraph &h = g->g;
    if (h.R == 0 || h.R > 64) throw ArgError("max_nbrs must be 1..64 for the device search");
    if (h.has_overlay && (h.upper_R == 0 || h.upper_R > 64)) throw ArgError("overlay degree must be 1..64");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    scratch_drain(ix);
    auto up = [&](DevBuf &b, const void *src, size_t bytes) {
      b.release();
      b.reserve(std::max<size_t>(bytes, 4));
      if (bytes)
        hip_check(hipMemcpyAsync(b.ptr, src, bytes, hipMemcpyHostToDevice, ix->stream), "upload graph");
    };
    // rows of a HNSW adjacency list never repeat an id; scan once so the kernel can skip dedup.
    bool dup = false;
    for (uint64_t i = 0; i < h.n && !dup; ++i) {
      const uint32_t *r = &h.l0[i * h.R];
      for (uint32_t a = 0; a < h.R && r[a] != 0xffffffffu && !dup; ++a)
        for (uint32_t b = 0; b < a; ++b)
          if (r[a] == r[b]) {
            dup = true;
            break;
          }
    }
    up(ix->l0, h.l0.data(), h.l0.size() * 4);
    up(ix->levels, h.levels.data(), h.levels.size() * 4);
    up(ix->upper_off, h.upper_off.data(), h.upper_off.size() * 8);
    up(ix->upper_edges, h.upper_edges.data(), h.upper_edges.size() * 4);
    up(ix->eps, h.eps.data(), h.eps.size() * 4);
    hip_check(hipStreamSynchronize(ix->stream), "sync");
    ix->R = h.R;
    ix->upper_R = h.upper_R;
    ix->ep = h.ep;
    ix->n_eps = static_cast<uint32_t>(h.eps.size());
    ix->has_overlay = h.has_overlay;
    ix->dedup = dup;
    ix->graph_n = h.n;
    ix->has_graph = true;
    ix->upd_graph.reset();
    ix->upd_rows.reset();
    ix->upd_ctx.reset();
  });
}

// ---- device mirror patches (online updates) ------------------------------------------------
namespace {

// Grow a device buffer to `bytes`, keeping its first `keep` bytes.
void grow_keep(alaya_index *ix, DevBuf &b, size_t bytes, size_t keep) {
  if (bytes <= b.bytes) return;
  DevBuf nb;
  nb.reserve(bytes);
  hip_check(hipMemsetAsync(nb.ptr, 0, nb.bytes, ix->stream), "memset");
  if (keep && b.ptr) hip_check(hipMemcpyAsync(nb.ptr, b.ptr, keep, hipMemcpyDeviceToDevice, ix->stream), "copy");
  hip_check(hipStreamSynchronize(ix->stream), "sync");
  std::swap(b.ptr, nb.ptr);
  std::swap(b.bytes, nb.bytes);
}

void reserve_locked(alaya_index *ix, uint64_t capacity) {
  if (!ix->base.ptr) throw ArgError("index has no base vectors");
  if (capacity < ix->n) throw ArgError("capacity below the stored rows");
  const size_t row = static_cast<size_t>(ix->stride) * 4;
  grow_keep(ix, ix->base, std::max<uint64_t>(capacity, 1) * row, ix->n * row);
  const size_t words = (std::max<uint64_t>(capacity, 1) + 31) / 32;
  if (!ix->has_valid) {  // all stored rows valid: materialise the bitmap so rows can be removed
    std::vector<uint32_t> w(words, 0u);
    for (uint64_t i = 0; i < ix->n; ++i) w[i >> 5] |= 1u << (i & 31);
    ix->valid.release();
    ix->valid.reserve(words * 4);
    hip_check(hipMemcpyAsync(ix->valid.ptr, w.data(), words * 4, hipMemcpyHostToDevice, ix->stream), "bitmap");
    hip_check(hipStreamSynchronize(ix->stream), "sync");
    ix->has_valid = true;
  } else {
    grow_keep(ix, ix->valid, words * 4, (ix->n + 31) / 32 * 4);
  }
  if (ix->has_graph) {
    grow_keep(ix, ix->l0, std::max<uint64_t>(capacity, 1) * ix->R * 4, ix->graph_n * ix->R * 4);
    grow_keep(ix, ix->levels, std::max<uint64_t>(capacity, 1) * 4, ix->graph_n * 4);
    grow_keep(ix, ix->upper_off, std::max<uint64_t>(capacity, 1) * 8, ix->graph_n * 8);
  }
  ix->capacity = std::max(ix->capacity, capacity);
}

// The three patch helpers below change buffers an in-flight search reads (rows, adjacency, the
// validity bitmap), so each first waits for every earlier launch on the index (alaya_hip.h's
// stream contract: a call is ordered after the launches before it).
void write_rows_locked(alaya_index *ix, uint64_t first, const float *rows, uint64_t count) {
  scratch_drain(ix);
  const size_t row = static_cast<size_t>(ix->stride) * 4;
  if (first + count > ix->capacity || (first + count) * row > ix->base.bytes)
    throw ArgError("rows beyond the reserved capacity");
  char *dst = static_cast<char *>(ix->base.ptr) + first * row;
  hip_check(hipMemset2DAsync(dst, row, 0, row, count, ix->stream), "memset");
  hip_check(hipMemcpy2DAsync(dst, row, rows, static_cast<size_t>(ix->dim) * 4, static_cast<size_t>(ix->dim) * 4,
                             count, hipMemcpyHostToDevice, ix->stream), "write rows");
  hip_check(hipStreamSynchronize(ix->stream), "sync");
  ix->n = std::max(ix->n, first + count);
  ix->norms_ready = false;
  ix->tiles_ready = false;
  // the screening copies follow the written rows; rows past what one holds mark it for a rebuild
  for (uint32_t format = 1; format <= 2; ++format) {
    alaya_index::ScreenCopy &c = ix->screen_copy[format - 1];
    if (!c.ready) continue;
    if (first + count <= c.cap) {
      screen_fill(ix, format, first, count, ix->stream);
      hip_check(hipStreamSynchronize(ix->stream), "sync");
    } else {
      c.ready = false;
    }
  }
}

void write_edges_locked(alaya_index *ix, const uint32_t *ids, const uint32_t *edges, uint64_t count) {
  if (!ix->has_graph) throw ArgError("index has no graph");
  scratch_drain(ix);
  for (uint64_t i = 0; i < count; ++i) {
    if (ids[i] >= ix->capacity || ids[i] >= ix->n || (static_cast<uint64_t>(ids[i]) + 1) * ix->R * 4 > ix->l0.bytes ||
        (ix->has_overlay && (static_cast<uint64_t>(ids[i]) + 1) * 4 > ix->levels.bytes))
      throw ArgError("edge row id out of range (reserve capacity first)");
    const uint32_t *r = edges + i * ix->R;
    for (uint32_t a = 0; a < ix->R && r[a] != 0xffffffffu; ++a) {
      for (uint32_t b = 0; b < a; ++b)
        if (r[a] == r[b]) ix->dedup = true;  // e.g. the zero padding update() writes
    }
    hip_check(hipMemcpyAsync(ix->l0.as<uint32_t>() + static_cast<uint64_t>(ids[i]) * ix->R, r, ix->R * 4,
                             hipMemcpyHostToDevice, ix->stream), "write edges");
    ix->graph_n = std::max<uint64_t>(ix->graph_n, static_cast<uint64_t>(ids[i]) + 1);
  }
  hip_check(hipStreamSynchronize(ix->stream), "sync");
}

void set_valid_locked(alaya_index *ix, uint64_t id, bool valid) {
  if (!ix->has_valid || id >= ix->capacity || (id / 32 + 1) * 4 > ix->valid.bytes)
    throw ArgError("id out of range (reserve capacity first)");
  scratch_drain(ix);
  uint32_t w = 0;
  uint32_t *dw = ix->valid.as<uint32_t>() + (id >> 5);
  hip_check(hipMemcpy(&w, dw, 4, hipMemcpyDeviceToHost), "read bitmap");
  w = valid ? (w | (1u << (id & 31))) : (w & ~(1u << (id & 31)));
  hip_check(hipMemcpy(dw, &w, 4, hipMemcpyHostToDevice), "write bitmap");
  ix->tiles_ready = false;  // the records carry +inf norms for cleared rows
}

}  // namespace

int alaya_index_reserve(alaya_index *ix, uint64_t capacity) {
  return guarded([&] {
    if (!ix) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    scratch_drain(ix);
    reserve_locked(ix, capacity);
  });
}

int alaya_index_write_rows(alaya_index *ix, uint64_t first, const float *rows, uint64_t count) {
  return guarded([&] {
    if (!ix || (count && !rows)) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    write_rows_locked(ix, first, rows, count);
  });
}

int alaya_index_write_edges(alaya_index *ix, const uint32_t *ids, const uint32_t *edges, uint64_t count) {
  return guarded([&] {
    if (!ix || (count && (!ids || !edges))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    write_edges_locked(ix, ids, edges, count);
  });
}

int alaya_index_set_valid(alaya_index *ix, uint64_t id, int valid) {
  return guarded([&] {
    if (!ix) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    set_valid_locked(ix, id, valid != 0);
  });
}

int alaya_index_enable_updates(alaya_index *ix, const alaya_graph *g, const float *rows, uint64_t n,
                               uint64_t capacity, const uint8_t *valid_bitmap) {
  return guarded([&] {
    if (!ix || !g || (n && !rows)) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (g->g.n != n || ix->n != n || ix->graph_n != n) throw ArgError("graph, rows and device index sizes differ");
    if (capacity < n) throw ArgError("capacity below the stored rows");
    scratch_drain(ix);
    auto m = std::make_unique<alaya_amd::RowMirror>();
    m->dim = ix->dim;
    m->metric = ix->metric | (ix->generic ? ALAYA_DIST_GENERIC : 0);
    m->rows.assign(rows, rows + n * ix->dim);
    m->valid.assign((capacity + 7) / 8 + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
      const bool v = valid_bitmap ? ((valid_bitmap[i >> 3] >> (i & 7)) & 1) : true;
      if (v) m->valid[i >> 3] |= static_cast<uint8_t>(1u << (i & 7));
    }
    ix->upd_graph = std::make_unique<alaya_amd::HostGraph>(g->g);
    ix->upd_rows = std::move(m);
    ix->upd_ctx = std::make_unique<alaya_amd::UpdateContext>();
    reserve_locked(ix, capacity);
  });
}

int alaya_index_insert(alaya_index *ix, const float *search_query, const float *row, uint32_t ef,
                       uint64_t *new_id) {
  return guarded_scratch(ix, [&] {
    if (!ix || !search_query || !row || !new_id) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (!ix->upd_graph) throw ArgError("updates are not enabled on this index");
    alaya_amd::HostGraph &g = *ix->upd_graph;
    alaya_amd::RowMirror &m = *ix->upd_rows;
    alaya_amd::UpdateContext &ctx = *ix->upd_ctx;
    const uint32_t R = g.R;
    // search_solo(query, max_nbrs, results, ef) on the current index (graph_update_job.hpp:67-69)
    std::vector<uint32_t> results(R, 0u);
    ix->q_buf.reserve(static_cast<size_t>(ix->dim) * 4);
    ix->id_buf.reserve(static_cast<size_t>(R) * 4);
    hip_check(hipMemcpyAsync(ix->q_buf.ptr, search_query, ix->dim * 4, hipMemcpyHostToDevice, ix->stream), "H2D");
    do_search(ix, ix->q_buf.as<float>(), 1, R, std::max(ef, 1u), ix->id_buf.as<uint32_t>(), nullptr, nullptr,
              ix->stream);
    hip_check(hipMemcpyAsync(results.data(), ix->id_buf.ptr, R * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
    hip_check(hipStreamSynchronize(ix->stream), "insert search");
    // graph_->insert: -1 when the storage is full (then nothing else happens, :70-73)
    if (g.n >= ix->capacity) {
      *new_id = UINT64_MAX;
      return;
    }
    const uint32_t id = static_cast<uint32_t>(g.n);
    g.l0.insert(g.l0.end(), results.begin(), results.end());
    if (g.has_overlay) {  // Graph::insert adds a level-0 node; the overlay is not touched
      g.levels.push_back(0);
      g.upper_off.push_back(g.upper_edges.size());
    }
    g.n += 1;
    // space_->insert (RawSpace::insert: row stored, validity bit set)
    m.rows.insert(m.rows.end(), row, row + ix->dim);
    m.valid[id >> 3] |= static_cast<uint8_t>(1u << (id & 7));
    for (uint32_t i = 0; i < R; ++i)
      if (results[i] != 0xffffffffu) ctx.inserted_edges[results[i]].push_back(id);
    // update every node that gained an edge (:80-83), in the map's iteration order
    std::vector<uint32_t> touched{id};
    std::vector<uint32_t> edges(results);
    for (const auto &kv : ctx.inserted_edges) {
      std::vector<uint32_t> e = alaya_amd::update_edges(g, m, ctx, kv.first);
      std::copy(e.begin(), e.end(), g.l0.begin() + static_cast<size_t>(kv.first) * R);
      touched.push_back(kv.first);
      edges.insert(edges.end(), e.begin(), e.end());
    }
    ctx.inserted_edges.clear();
    // mirror into HBM: the row, its validity bit, the new and the updated adjacency rows
    write_rows_locked(ix, id, row, 1);
    set_valid_locked(ix, id, true);
    write_edges_locked(ix, touched.data(), edges.data(), touched.size());
    *new_id = id;
  });
}

int alaya_index_remove(alaya_index *ix, uint64_t id) {
  return guarded([&] {
    if (!ix) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (!ix->upd_graph) throw ArgError("updates are not enabled on this index");
    if (id >= ix->upd_graph->n) throw ArgError("id out of range");
    alaya_amd::record_remove(*ix->upd_graph, *ix->upd_ctx, static_cast<uint32_t>(id));
    ix->upd_rows->valid[id >> 3] &= static_cast<uint8_t>(~(1u << (id & 7)));
    set_valid_locked(ix, id, false);
  });
}

int alaya_index_export_graph(alaya_index *ix, alaya_graph **out) {
  return guarded([&] {
    if (!ix || !out) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->upd_graph) throw ArgError("updates are not enabled on this index");
    *out = new alaya_graph{*ix->upd_graph};
  });
}

int alaya_index_export_rows(alaya_index *ix, float *rows, uint8_t *valid_bitmap, uint64_t *n) {
  return guarded([&] {
    if (!ix || !n) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->upd_rows) throw ArgError("updates are not enabled on this index");
    *n = ix->upd_graph->n;
    if (rows) std::memcpy(rows, ix->upd_rows->rows.data(), ix->upd_rows->rows.size() * 4);
    if (valid_bitmap) std::memcpy(valid_bitmap, ix->upd_rows->valid.data(), (*n + 7) / 8);
  });
}

}  // extern "C"

// ---- device graph construction ----------------------------------------------------------------
namespace {

// One launch group of the batched build: the points of batch [first, ...) active at `level`.
struct BuildStep {
  uint32_t first;
  int level;
  int max_level;  // graph max level before the batch
  uint32_t ep;    // graph entry point before the batch
  uint64_t off;   // active points: act[off, off + cnt)
  uint32_t cnt;
  int refine;     // level-0 refine pass of the batch
};

// Batch schedule (label order): batch size max(1, min(max_batch, inserted / batch_div)); a point
// whose level exceeds the graph's max level closes its batch, so the entry point / max level a
// batch sees are exactly the sequential ones (hnswlib.hpp:740-748).
// The schedule of rows [start, n) of a graph that holds rows [0, start) with entry point `ep` (whose
// level is the graph's max level): a build from scratch is start = 1, ep = 0.  The batch size
// depends on the rows inserted so far only, so a schedule continued from one of its own batch
// boundaries is the rest of the whole schedule.  `ends` (optional) receives every batch's end.
std::vector<BuildStep> build_schedule(const uint32_t *lv, uint64_t n, uint64_t start, uint32_t ep, uint32_t batch_div,
                                      uint32_t max_batch, uint32_t refine, std::vector<uint32_t> &act,
                                      uint32_t *final_ep, int *final_max, std::vector<uint64_t> *ends = nullptr) {
  std::vector<BuildStep> steps;
  int maxl = n ? static_cast<int>(lv[ep]) : 0;
  uint64_t i = start;
  while (i < n) {
    const uint64_t b = std::max<uint64_t>(1, std::min<uint64_t>(max_batch, i / batch_div));
    uint64_t end = std::min<uint64_t>(n, i + b);
    int top = 0;
    for (uint64_t j = i; j < end; ++j) {
      top = std::max(top, std::min(static_cast<int>(lv[j]), maxl));
      if (static_cast<int>(lv[j]) > maxl) {
        end = j + 1;
        break;
      }
    }
    for (int L = top; L >= 0; --L) {
      BuildStep st{static_cast<uint32_t>(i), L, maxl, ep, act.size(), 0, 0};
      for (uint64_t j = i; j < end; ++j)
        if (std::min(static_cast<int>(lv[j]), maxl) >= L) act.push_back(static_cast<uint32_t>(j));
      st.cnt = static_cast<uint32_t>(act.size() - st.off);
      steps.push_back(st);
    }
    // refine passes over level 0 (single-point batches have no batch mates to find)
    for (uint32_t r = 0; r < refine && end - i > 1; ++r) {
      BuildStep st = steps.back();
      st.refine = 1;
      steps.push_back(st);
    }
    if (static_cast<int>(lv[end - 1]) > maxl) {
      ep = static_cast<uint32_t>(end - 1);
      maxl = static_cast<int>(lv[end - 1]);
    }
    if (ends) ends->push_back(end);
    i = end;
  }
  *final_ep = ep;
  *final_max = maxl;
  return steps;
}

// What a run of build steps reports (alaya_index_build_graph's stats, steps of this run only).
struct BuildRun {
  uint64_t batches = 0, launches = 0;
  unsigned long long counters[8] = {0};  // [0] prunes, [1] appends, [2] heuristic distances
  float ms = 0.f;
  uint32_t bmax = 1;
  void write(uint64_t *stats, int max_level) const {
    if (!stats) return;
    stats[0] = batches;
    stats[1] = launches;
    stats[2] = counters[0];
    stats[3] = counters[1];
    stats[4] = counters[2];
    stats[5] = static_cast<uint64_t>(ms * 1000.0);
    stats[6] = bmax;
    stats[7] = static_cast<uint64_t>(max_level);
  }
};

// Run `steps` (build_schedule; `act` their active points) on the index's device graph: rows, levels,
// upper_off and empty adjacency slots of every scheduled point are in HBM, ix->n covers them.
// tombstones: the validity bitmap has cleared bits -- the searches measure those rows as a query does
// (FLT_MAX) and the selection drops them (launch_build_select).  duplicates: adjacency rows may
// repeat an id (launch_build_apply).  `before_sync` queues the caller's downloads behind the steps;
// the call returns after the stream has drained.
template <typename F>
BuildRun run_build_steps(alaya_index *ix, uint32_t R, uint32_t ef, uint32_t max_batch,
                         const std::vector<BuildStep> &steps, const std::vector<uint32_t> &act, bool tombstones,
                         bool duplicates, F &&before_sync) {
  const uint32_t M = R / 2;  // hnsw_builder.hpp:71-72: M = R/2, M0 = R
  hipStream_t st = ix->stream;
  BuildRun run;
  for (const BuildStep &s : steps) run.bmax = std::max(run.bmax, s.cnt);
  const uint32_t bmax = run.bmax;
  hipEvent_t e0, e1;
  hip_check(hipEventCreate(&e0), "event");
  hip_check(hipEventCreate(&e1), "event");
  DevBuf d_act, d_next, c_ids, c_d, c_n, k_in, k_out, dd_in, dd_out, sort_tmp, cnt;
  d_act.reserve(std::max<size_t>(act.size(), 1) * 4);
  if (!act.empty())
    hip_check(hipMemcpyAsync(d_act.ptr, act.data(), act.size() * 4, hipMemcpyHostToDevice, st), "H2D");
  d_next.reserve(static_cast<size_t>(max_batch) * 4);
  c_ids.reserve(static_cast<size_t>(bmax) * ef * 4);
  c_d.reserve(static_cast<size_t>(bmax) * ef * 4);
  c_n.reserve(static_cast<size_t>(bmax) * 4);
  const size_t n_edge_max = static_cast<size_t>(bmax) * M;
  k_in.reserve(n_edge_max * 8);
  k_out.reserve(n_edge_max * 8);
  dd_in.reserve(n_edge_max * 4);
  dd_out.reserve(n_edge_max * 4);
  size_t tmp_bytes = 0;
  hip_check(alaya_amd::sort_edges(nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, n_edge_max, st), "sort size");
  sort_tmp.reserve(tmp_bytes);
  cnt.reserve(8 * 8);
  hip_check(hipMemsetAsync(cnt.ptr, 0, 8 * 8, st), "memset");
  ix->work.reserve(4);

  alaya_amd::BuildParams bp{};
  bp.s = base_params(ix);
  if (!tombstones) bp.s.valid = nullptr;
  bp.s.l0 = ix->l0.as<uint32_t>();
  bp.s.R = R;
  bp.s.levels = ix->levels.as<uint32_t>();
  bp.s.upper_off = ix->upper_off.as<uint64_t>();
  bp.s.upper_edges = ix->upper_edges.as<uint32_t>();
  bp.s.upper_R = R;
  bp.s.queries = nullptr;
  bp.s.ef = ef;
  bp.s.work_counter = ix->work.as<uint32_t>();
  bp.l0w = ix->l0.as<uint32_t>();
  bp.upw = ix->upper_edges.as<uint32_t>();
  bp.next = d_next.as<uint32_t>();
  bp.cand_ids = c_ids.as<uint32_t>();
  bp.cand_d = c_d.as<float>();
  bp.cand_n = c_n.as<uint32_t>();
  bp.M = M;
  bp.counters = cnt.as<unsigned long long>();
  // visited-set sizing and the spill area for the largest batch (sized once: kernels in flight)
  {
    SearchParams probe = bp.s;
    const uint32_t hl = size_visited(ix, probe, alaya_amd::resolve_search_variant({ix->dim, probe.ip, 0, ix->generic, 0}),
                                     bmax, ef);
    const size_t lds = alaya_amd::build_lds_bytes(ix->stride, ef, hl, probe.vis_rbits != alaya_amd::kVisWide);
    bp.s.hash_log2 = hl;
    bp.s.vis_rbits = probe.vis_rbits;
    bp.s.vis_lbits = probe.vis_lbits;
    bp.s.vis_max_disp = probe.vis_max_disp;
    bp.s.vis_limit = probe.vis_limit;
    if (lds > kLdsPerCu) throw ArgError("ef_construction / dim too large for the LDS budget");
  }
  const size_t lds = alaya_amd::build_lds_bytes(ix->stride, ef, bp.s.hash_log2, bp.s.vis_rbits != alaya_amd::kVisWide);
  int per_cu = 0;
  hip_check(alaya_amd::build_search_occupancy(bp, lds, &per_cu), "occupancy");
  per_cu = std::max(1, per_cu);
  const uint64_t grid_max = static_cast<uint64_t>(per_cu) * ix->num_cus;
  prepare_spill(ix, bp.s, std::min<uint64_t>(grid_max, bmax), st);

  hip_check(hipEventRecord(e0, st), "event");
  for (const BuildStep &s : steps) {
    bp.s.nq = s.cnt;
    bp.s.ep = s.ep;
    bp.pts = d_act.as<uint32_t>() + s.off;
    bp.batch_first = s.first;
    bp.level = s.level;
    bp.max_level = s.max_level;
    bp.refine = s.refine;
    bp.Mmax = s.level == 0 ? R : M;
    bp.edge_keys = k_in.as<uint64_t>();
    bp.edge_d = dd_in.as<float>();
    const int grid = static_cast<int>(std::min<uint64_t>(s.cnt, grid_max));
    const int wide = static_cast<int>(std::min<uint64_t>(s.cnt, static_cast<uint64_t>(ix->num_cus) * 16));
    hip_check(hipMemsetAsync(bp.s.work_counter, 0, 4, st), "memset");
    hip_check(alaya_amd::launch_build_search(bp, grid, lds, st), "build search");
    hip_check(alaya_amd::launch_build_select(bp, wide, st, tombstones), "build select");
    const uint64_t ne = static_cast<uint64_t>(s.cnt) * M;
    size_t tb = tmp_bytes;
    hip_check(alaya_amd::sort_edges(sort_tmp.ptr, &tb, k_in.as<uint64_t>(), k_out.as<uint64_t>(), dd_in.as<float>(),
                                    dd_out.as<float>(), ne, st), "sort edges");
    bp.edge_keys = k_out.as<uint64_t>();
    bp.edge_d = dd_out.as<float>();
    bp.n_edges = ne;
    const int agrid = static_cast<int>(std::min<uint64_t>((ne + 63) / 64, static_cast<uint64_t>(ix->num_cus) * 16));
    hip_check(alaya_amd::launch_build_apply(bp, agrid, st, duplicates), "build apply");
    run.launches += 4;
  }
  hip_check(hipEventRecord(e1, st), "event");
  before_sync();
  hip_check(hipMemcpyAsync(run.counters, cnt.ptr, sizeof(run.counters), hipMemcpyDeviceToHost, st), "D2H");
  hip_check(hipStreamSynchronize(st), "device build");
  hip_check(hipEventElapsedTime(&run.ms, e0, e1), "event");
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  run.batches = steps.empty() ? 0 : 1;
  for (size_t i = 1; i < steps.size(); ++i) run.batches += steps[i].first != steps[i - 1].first ? 1 : 0;
  return run;
}

// The device graph's l0 and overlay rows into a host graph whose levels and offsets the caller set.
void queue_graph_download(alaya_index *ix, HostGraph &g, uint64_t n_upper) {
  g.l0.resize(g.n * g.R);
  g.upper_edges.resize(n_upper);
  hip_check(hipMemcpyAsync(g.l0.data(), ix->l0.ptr, g.n * g.R * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
  if (n_upper)
    hip_check(hipMemcpyAsync(g.upper_edges.data(), ix->upper_edges.ptr, n_upper * 4, hipMemcpyDeviceToHost,
                             ix->stream), "D2H");
}

}  // namespace

extern "C" {

int alaya_index_build_graph(alaya_index *ix, uint32_t R, uint32_t ef_construction, uint64_t seed,
                            uint32_t batch_div, uint32_t max_batch, uint32_t refine, alaya_graph **out,
                            uint64_t *stats) {
  return guarded_scratch(ix, [&] {
    if (!ix) throw ArgError("invalid arguments");
    if (R < 2 || R > 64 || R % 2) throw ArgError("max_nbrs must be even and in 2..64 for the device build");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    scratch_drain(ix);
    if (!ix->base.ptr || ix->n == 0) throw ArgError("index has no base vectors");
    if (ix->n >= (1ull << 31)) throw ArgError("ids must stay below 2^31 (LinearPool checked bit)");
    const uint64_t n = ix->n;
    const uint32_t M = R / 2;                            // hnsw_builder.hpp:71-72: M = R/2, M0 = R
    const uint32_t ef = std::max(ef_construction, M);    // hnswlib.hpp:104
    batch_div = batch_div ? batch_div : 16;
    max_batch = max_batch ? max_batch : 65536;
    hipStream_t st = ix->stream;

    // levels and overlay offsets are known up front (upper lists R wide, HNSWBuilder's export)
    const std::vector<uint32_t> lv = alaya_amd::hnsw_levels(n, M, seed);
    std::vector<uint64_t> off(n);
    uint64_t n_upper = 0;
    for (uint64_t i = 0; i < n; ++i) {
      off[i] = n_upper;
      n_upper += static_cast<uint64_t>(lv[i]) * R;
    }
    // the build is an extension of the one-row graph {row 0}
    std::vector<uint32_t> act;
    uint32_t ep = 0;
    int maxl = 0;
    const std::vector<BuildStep> steps = build_schedule(lv.data(), n, 1, 0, batch_div, max_batch, refine, act, &ep, &maxl);

    // device graph (installed as the index's search graph)
    ix->has_graph = false;
    ix->upd_graph.reset();
    ix->upd_rows.reset();
    ix->upd_ctx.reset();
    ix->l0.release();
    ix->l0.reserve(n * R * 4);
    ix->levels.release();
    ix->levels.reserve(n * 4);
    ix->upper_off.release();
    ix->upper_off.reserve(n * 8);
    ix->upper_edges.release();
    ix->upper_edges.reserve(std::max<uint64_t>(n_upper, 1) * 4);
    hip_check(hipMemsetAsync(ix->l0.ptr, 0xff, n * R * 4, st), "memset");
    if (n_upper) hip_check(hipMemsetAsync(ix->upper_edges.ptr, 0xff, n_upper * 4, st), "memset");
    hip_check(hipMemcpyAsync(ix->levels.ptr, lv.data(), n * 4, hipMemcpyHostToDevice, st), "H2D");
    hip_check(hipMemcpyAsync(ix->upper_off.ptr, off.data(), n * 8, hipMemcpyHostToDevice, st), "H2D");

    HostGraph g;
    g.n = n;
    g.R = R;
    g.has_overlay = true;
    g.upper_R = R;
    g.ep = ep;
    g.levels = lv;
    g.upper_off = off;
    const BuildRun run = run_build_steps(ix, R, ef, max_batch, steps, act, false, false,
                                         [&] { queue_graph_download(ix, g, n_upper); });
    ix->R = R;
    ix->upper_R = R;
    ix->ep = ep;
    ix->n_eps = 0;
    ix->has_overlay = true;
    ix->dedup = false;
    ix->graph_n = n;
    ix->has_graph = true;
    run.write(stats, maxl);
    if (out) *out = new alaya_graph{std::move(g)};
  });
}

int alaya_build_batches(const uint32_t *levels, uint64_t n, uint64_t start, uint32_t ep, uint32_t batch_div,
                        uint32_t max_batch, uint64_t *ends, uint64_t *n_batches) {
  return guarded([&] {
    if ((n && !levels) || !n_batches) throw ArgError("invalid arguments");
    if (start == 0 || start > n || ep >= start) throw ArgError("start must be in 1..n and the entry point below it");
    std::vector<uint32_t> act;
    std::vector<uint64_t> e;
    uint32_t fep = 0;
    int fmax = 0;
    build_schedule(levels, n, start, ep, batch_div ? batch_div : 16, max_batch ? max_batch : 65536, 0, act, &fep, &fmax,
                   &e);
    *n_batches = e.size();
    if (ends) std::copy(e.begin(), e.end(), ends);
  });
}

int alaya_index_extend_graph(alaya_index *ix, const float *rows, uint64_t count, uint32_t ef_construction,
                             uint64_t seed, uint32_t batch_div, uint32_t max_batch, uint32_t refine,
                             alaya_graph **out, uint64_t *stats) {
  return guarded_scratch(ix, [&] {
    if (!ix || (count && !rows)) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    scratch_drain(ix);
    // every refusal comes before the first change to the index
    if (!ix->base.ptr || ix->n == 0) throw ArgError("index has no base vectors");
    if (!ix->has_graph || ix->graph_n != ix->n) throw ArgError("index has no graph over its rows");
    if (!ix->has_overlay || ix->upper_R != ix->R)
      throw ArgError("the device build extends HNSW graphs whose overlay lists are max_nbrs wide");
    const uint32_t R = ix->R;
    if (R < 2 || R > 64 || R % 2) throw ArgError("max_nbrs must be even and in 2..64 for the device build");
    const uint64_t n0 = ix->n, n = n0 + count;
    if (n >= (1ull << 31)) throw ArgError("ids must stay below 2^31 (LinearPool checked bit)");
    if (ix->upd_graph && ix->upd_graph->n != n0) throw ArgError("the update mirror and the device index differ");
    const uint32_t M = R / 2;
    const uint32_t ef = std::max(ef_construction, M);
    batch_div = batch_div ? batch_div : 16;
    max_batch = max_batch ? max_batch : 65536;
    hipStream_t st = ix->stream;

    // the graph's own levels and offsets; the new rows take the tail of the draw for n rows (a
    // sequential draw: its first n0 levels are the draw for n0 rows) and overlay slots past the end
    std::vector<uint32_t> lv(n);
    std::vector<uint64_t> off(n);
    hip_check(hipMemcpyAsync(lv.data(), ix->levels.ptr, n0 * 4, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemcpyAsync(off.data(), ix->upper_off.ptr, n0 * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "read levels");
    uint64_t n_upper0 = 0;
    for (uint64_t i = 0; i < n0; ++i)
      if (lv[i]) n_upper0 = std::max(n_upper0, off[i] + static_cast<uint64_t>(lv[i]) * R);
    if (n_upper0 * 4 > ix->upper_edges.bytes || ix->ep >= n0) throw ArgError("the installed graph is inconsistent");
    uint64_t n_upper = n_upper0;
    if (count) {
      const std::vector<uint32_t> draw = alaya_amd::hnsw_levels(n, M, seed);
      for (uint64_t i = n0; i < n; ++i) {
        lv[i] = draw[i];
        off[i] = n_upper;
        n_upper += static_cast<uint64_t>(lv[i]) * R;
      }
    }
    std::vector<uint32_t> act;
    uint32_t ep = ix->ep;
    int maxl = static_cast<int>(lv[ep]);
    const std::vector<BuildStep> steps =
        build_schedule(lv.data(), n, n0, ix->ep, batch_div, max_batch, refine, act, &ep, &maxl);

    // removed rows: the bitmap travels with the build only when a bit of [0, n0) is clear
    bool tombstones = false;
    if (ix->has_valid) {
      std::vector<uint32_t> w((n0 + 31) / 32);
      hip_check(hipMemcpy(w.data(), ix->valid.ptr, w.size() * 4, hipMemcpyDeviceToHost), "read bitmap");
      for (uint64_t i = 0; i < n0 && !tombstones; ++i) tombstones = !((w[i >> 5] >> (i & 31)) & 1u);
    }

    // grow every per-row buffer once, then write the rows, their bits, codes and empty graph slots
    const size_t row = static_cast<size_t>(ix->stride) * 4;
    grow_keep(ix, ix->base, n * row, n0 * row);
    if (ix->has_valid) grow_keep(ix, ix->valid, (n + 31) / 32 * 4, (n0 + 31) / 32 * 4);
    grow_keep(ix, ix->l0, n * R * 4, n0 * R * 4);
    grow_keep(ix, ix->levels, n * 4, n0 * 4);
    grow_keep(ix, ix->upper_off, n * 8, n0 * 8);
    grow_keep(ix, ix->upper_edges, std::max<uint64_t>(n_upper, 1) * 4, n_upper0 * 4);
    if (ix->has_sq8) grow_keep(ix, ix->codes, n * ix->code_stride, n0 * ix->code_stride);
    ix->capacity = std::max(ix->capacity, n);
    if (count) {
      write_rows_locked(ix, n0, rows, count);  // ix->n = n; norms, tiles and screen copies follow
      if (ix->has_valid) {
        hip_check(alaya_amd::launch_set_valid_range(ix->valid.as<uint32_t>(), n0, count, st), "set valid");
        ix->tiles_ready = false;
      }
      if (ix->has_sq8)
        hip_check(alaya_amd::launch_sq8_encode_rows(ix->base.as<float>(), ix->stride, ix->dim, ix->sq_min.as<float>(),
                                                    ix->sq_max.as<float>(), ix->codes.as<uint8_t>(), ix->code_stride,
                                                    n0, count, st), "sq8 encode");
      hip_check(hipMemsetAsync(ix->l0.as<uint32_t>() + n0 * R, 0xff, count * R * 4, st), "memset");
      if (n_upper > n_upper0)
        hip_check(hipMemsetAsync(ix->upper_edges.as<uint32_t>() + n_upper0, 0xff, (n_upper - n_upper0) * 4, st), "memset");
      hip_check(hipMemcpyAsync(ix->levels.as<uint32_t>() + n0, lv.data() + n0, count * 4, hipMemcpyHostToDevice, st), "H2D");
      hip_check(hipMemcpyAsync(ix->upper_off.as<uint64_t>() + n0, off.data() + n0, count * 8, hipMemcpyHostToDevice, st),
                "H2D");
    }
    ix->graph_n = n;

    HostGraph g;
    g.n = n;
    g.R = R;
    g.has_overlay = true;
    g.upper_R = R;
    g.ep = ep;
    g.levels = lv;
    g.upper_off = off;
    BuildRun run;
    try {
      run = run_build_steps(ix, R, ef, max_batch, steps, act, tombstones, ix->dedup,
                            [&] { queue_graph_download(ix, g, n_upper); });
    } catch (const ArgError &) {  // refused before its first launch (the LDS budget): the rows are not added
      ix->n = n0;
      ix->graph_n = n0;
      throw;
    }
    ix->ep = ep;
    if (ix->upd_graph) {  // the mirror follows; the record of pending removals (upd_ctx) stays
      *ix->upd_graph = g;
      alaya_amd::RowMirror &m = *ix->upd_rows;
      m.rows.insert(m.rows.end(), rows, rows + count * ix->dim);
      if (m.valid.size() < (ix->capacity + 7) / 8 + 1) m.valid.resize((ix->capacity + 7) / 8 + 1, 0);
      for (uint64_t i = n0; i < n; ++i) m.valid[i >> 3] |= static_cast<uint8_t>(1u << (i & 7));
    }
    run.write(stats, maxl);
    if (out) *out = new alaya_graph{std::move(g)};
  });
}

int alaya_index_read_sq8(alaya_index *ix, uint64_t first, uint64_t count, uint8_t *codes) {
  return guarded([&] {
    if (!ix || (count && !codes)) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (!ix->has_sq8) throw ArgError("index has no SQ8 codes");
    if (first + count > ix->n || (first + count) * ix->code_stride > ix->codes.bytes) throw ArgError("rows out of range");
    if (!count) return;
    hip_check(hipMemcpy2DAsync(codes, ix->dim, ix->codes.as<uint8_t>() + first * ix->code_stride, ix->code_stride,
                               ix->dim, count, hipMemcpyDeviceToHost, ix->stream), "read codes");
    hip_check(hipStreamSynchronize(ix->stream), "read codes");
  });
}

int alaya_index_batch_search_device(alaya_index *ix, const float *d_queries, uint64_t nq,
                                    uint32_t k, uint32_t ef, uint32_t *d_ids, float *d_dists,
                                    uint32_t *d_counters, void *stream) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_ids))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    do_search(ix, d_queries, nq, k, ef, d_ids, d_dists, d_counters,
              static_cast<hipStream_t>(stream));
  });
}

int alaya_index_shard_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k,
                                    uint32_t ef, uint32_t *d_ids, float *d_dists, uint32_t *d_counters,
                                    void *stream) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_ids || !d_dists))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    do_search(ix, d_queries, nq, k, ef, d_ids, d_dists, d_counters, static_cast<hipStream_t>(stream), nullptr,
              false, 0xffffffffu);
  });
}

int alaya_index_batch_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                             uint32_t ef, uint32_t *ids, float *dists, uint32_t *counters) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!queries || !ids))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (nq == 0 || k == 0) return;
    const float *d_q = stage_queries(ix, queries, nq, k);
    do_search(ix, d_q, nq, k, ef, ix->id_buf.as<uint32_t>(), ix->dist_buf.as<float>(), ix->cnt_buf.as<uint32_t>(),
              ix->stream);
    fetch_results(ix, nq, k, ids, dists, counters);
    stream_sync(ix, "search");
  });
}

// alaya_index_filtered_search[_hop]_device / alaya_index_filtered_search[_hop]: one body each, hop = the through search
static int filtered_search_device_call(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k, uint32_t ef,
                                       const uint32_t *d_allow_words, uint32_t n_masks, const uint32_t *d_mask_of_query,
                                       uint32_t *d_ids, float *d_dists, uint32_t *d_counters, void *stream, bool hop,
                                       uint32_t *d_through) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_ids || !d_allow_words))) throw ArgError("invalid arguments");
    check_masks("filtered search", nq, n_masks, d_mask_of_query, false);
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    do_filtered_search(ix, d_queries, nq, k, ef, d_allow_words, d_mask_of_query, d_ids, d_dists, d_counters,
                       static_cast<hipStream_t>(stream), false, hop, d_through);
  });
}

int alaya_index_filtered_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k, uint32_t ef,
                                       const uint32_t *d_allow_words, uint32_t n_masks, const uint32_t *d_mask_of_query,
                                       uint32_t *d_ids, float *d_dists, uint32_t *d_counters, void *stream) {
  return filtered_search_device_call(ix, d_queries, nq, k, ef, d_allow_words, n_masks, d_mask_of_query, d_ids, d_dists,
                                     d_counters, stream, false, nullptr);
}

int alaya_index_filtered_search_hop_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k, uint32_t ef,
                                           const uint32_t *d_allow_words, uint32_t n_masks,
                                           const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists,
                                           uint32_t *d_counters, uint32_t *d_n_through, void *stream) {
  return filtered_search_device_call(ix, d_queries, nq, k, ef, d_allow_words, n_masks, d_mask_of_query, d_ids, d_dists,
                                     d_counters, stream, true, d_n_through);
}

static int filtered_search_host_call(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k, uint32_t ef,
                                     const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                     uint32_t *ids, float *dists, uint32_t *counters, bool hop, uint32_t *n_through) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!queries || !ids || !allow_words))) throw ArgError("invalid arguments");
    check_masks("filtered search", nq, n_masks, mask_of_query, true);
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (k == 0 || k > 224) throw ArgError("filtered search: k must be in 1..224");
    if (nq == 0) return;
    const bool through_out = hop && n_through;  // through_buf only for the through call that asks for the counts
    const float *d_q = stage_queries(ix, queries, nq, k);
    const uint32_t *d_allow = stage_masks(ix, allow_words, n_masks);
    const uint32_t *d_groups = stage_mask_indices(ix, mask_of_query, nq);
    if (through_out) ix->through_buf.reserve(nq * 4);
    do_filtered_search(ix, d_q, nq, k, ef, d_allow, d_groups, ix->id_buf.as<uint32_t>(), ix->dist_buf.as<float>(),
                       ix->cnt_buf.as<uint32_t>(), ix->stream, false, hop,
                       through_out ? ix->through_buf.as<uint32_t>() : nullptr);
    fetch_results(ix, nq, k, ids, dists, counters);
    if (through_out)
      hip_check(hipMemcpyAsync(n_through, ix->through_buf.ptr, nq * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
    stream_sync(ix, "filtered search");
  });
}

int alaya_index_filtered_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k, uint32_t ef,
                                const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                uint32_t *ids, float *dists, uint32_t *counters) {
  return filtered_search_host_call(ix, queries, nq, k, ef, allow_words, n_masks, mask_of_query, ids, dists, counters, false,
                                   nullptr);
}

int alaya_index_filtered_search_hop(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k, uint32_t ef,
                                    const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                    uint32_t *ids, float *dists, uint32_t *counters, uint32_t *n_through) {
  return filtered_search_host_call(ix, queries, nq, k, ef, allow_words, n_masks, mask_of_query, ids, dists, counters, true,
                                   n_through);
}

static void check_range_cap(uint32_t max_results) {
  if (max_results == 0 || max_results > alaya_amd::kRangeMaxCap)
    throw ArgError("range search: max_results must be in 1..4096");
}

// alaya_index_range_search_device / alaya_index_range_search: the search stage (do_filtered_search's range plan)
// into the index's append buffers, then the sort into d_ids / d_dists.  The caller holds ix->mu.
static void range_search_dev(alaya_index *ix, const float *d_q, uint64_t nq, uint32_t ef, const float *d_radii,
                             uint32_t max_results, const uint32_t *d_allow, const uint32_t *d_mask_of_query,
                             uint32_t *d_counts, uint32_t *d_ids, float *d_dists, uint32_t *d_cnt, hipStream_t s,
                             uint32_t max_frontier = 0, uint32_t *d_more = nullptr) {
  check_range_cap(max_results);
  const bool radius_mode = max_frontier != 0;  // (the radius entries refuse 0 themselves)
  if (ef == 0) throw ArgError("ef must be >= 1");
  alaya_amd::RangeMoreParams m{};
  if (radius_mode) {
    ix->range_frontier.reserve(static_cast<size_t>(nq) * max_frontier * 4);
    m.frontier_ids = ix->range_frontier.as<uint32_t>();
    m.cap = max_frontier;
    m.more = d_more;
  }
  const size_t slots = static_cast<size_t>(nq) * max_results;
  ix->range_ids.reserve(slots * 4);
  ix->range_d.reserve(slots * 4);
  alaya_amd::RangeParams r{};
  r.radii = d_radii;
  r.cap = max_results;
  r.append_ids = ix->range_ids.as<uint32_t>();
  r.append_dists = ix->range_d.as<float>();
  r.counts = d_counts;
  r.out_ids = d_ids;
  r.out_dists = d_dists;
  do_filtered_search(ix, d_q, nq, 0, ef, d_allow, d_mask_of_query, nullptr, nullptr, d_cnt, s, false, false, nullptr, &r,
                     radius_mode ? &m : nullptr);
  if (nq == 0) return;
  // diagnostics (ALAYA_RANGE_SORT=0, include/alaya_hip.h): the search stage alone, to time it; ids / dists are
  // then left unwritten
  if (const char *e = std::getenv("ALAYA_RANGE_SORT"))
    if (std::atoi(e) == 0) return;
  hip_check(alaya_amd::launch_range_sort(r, nq, s), "range sort launch");
  scratch_release(ix, s);  // the sort read the append buffers
}

// the range entries' mask arguments: none at all (no mask), or what the filtered entries accept
static void check_range_masks(uint64_t nq, const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                              bool host_indices) {
  if (!allow_words && n_masks == 0) {
    if (mask_of_query) throw ArgError("range search: mask_of_query without masks");
    return;
  }
  if (!allow_words) throw ArgError("range search: n_masks without allow_words");
  check_masks("range search", nq, n_masks, mask_of_query, host_indices);
}

static void check_range_frontier(bool radius_mode, uint32_t max_frontier) {
  if (radius_mode && (max_frontier == 0 || max_frontier > alaya_amd::kRangeMaxFrontier))
    throw ArgError("range search: max_frontier must be in 1..16384");
}

// The device entries of both modes (radius_mode: alaya_index_range_search_radius_device, else max_frontier = 0).
static int range_device_call(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t ef, const float *d_radii,
                             uint32_t max_results, const uint32_t *d_allow_words, uint32_t n_masks,
                             const uint32_t *d_mask_of_query, uint32_t *d_counts, uint32_t *d_ids, float *d_dists,
                             uint32_t *d_counters, void *stream, bool radius_mode, uint32_t max_frontier, uint32_t *d_more) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_radii || !d_counts || !d_ids || !d_dists))) throw ArgError("invalid arguments");
    check_range_masks(nq, d_allow_words, n_masks, d_mask_of_query, false);
    check_range_frontier(radius_mode, max_frontier);
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    range_search_dev(ix, d_queries, nq, ef, d_radii, max_results, d_allow_words, d_mask_of_query, d_counts, d_ids, d_dists,
                     d_counters, static_cast<hipStream_t>(stream), max_frontier, d_more);
  });
}

// The host entries of both modes; more (radius mode, nullable): nq x 2.
static int range_host_call(alaya_index *ix, const float *queries, uint64_t nq, uint32_t ef, const float *radii,
                           uint32_t max_results, const uint32_t *allow_words, uint32_t n_masks,
                           const uint32_t *mask_of_query, uint32_t *counts, uint32_t *ids, float *dists, uint32_t *counters,
                           bool radius_mode, uint32_t max_frontier, uint32_t *more) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!queries || !radii || !counts || !ids || !dists))) throw ArgError("invalid arguments");
    check_range_masks(nq, allow_words, n_masks, mask_of_query, true);
    for (uint64_t i = 0; i < nq; ++i)
      if (radii[i] != radii[i]) throw ArgError("range search: a radius is NaN");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    check_range_cap(max_results);  // (before the result buffers are sized by it)
    check_range_frontier(radius_mode, max_frontier);
    if (nq == 0) {
      range_search_dev(ix, nullptr, 0, ef, nullptr, max_results, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       ix->stream, max_frontier);  // the index's own refusals
      return;
    }
    const float *d_q = stage_queries(ix, queries, nq, max_results);
    const uint32_t *d_allow = allow_words ? stage_masks(ix, allow_words, n_masks) : nullptr;
    const uint32_t *d_groups = allow_words ? stage_mask_indices(ix, mask_of_query, nq) : nullptr;
    ix->range_radii.reserve(nq * 4);
    ix->range_cnt.reserve(nq * 4);
    const bool more_out = radius_mode && more;
    if (more_out) ix->range_more.reserve(nq * 8);
    hip_check(hipMemcpyAsync(ix->range_radii.ptr, radii, nq * 4, hipMemcpyHostToDevice, ix->stream), "upload radii");
    range_search_dev(ix, d_q, nq, ef, ix->range_radii.as<float>(), max_results, d_allow, d_groups,
                     ix->range_cnt.as<uint32_t>(), ix->id_buf.as<uint32_t>(), ix->dist_buf.as<float>(),
                     ix->cnt_buf.as<uint32_t>(), ix->stream, max_frontier, more_out ? ix->range_more.as<uint32_t>() : nullptr);
    fetch_results(ix, nq, max_results, ids, dists, counters);
    hip_check(hipMemcpyAsync(counts, ix->range_cnt.ptr, nq * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
    if (more_out) hip_check(hipMemcpyAsync(more, ix->range_more.ptr, nq * 8, hipMemcpyDeviceToHost, ix->stream), "D2H");
    stream_sync(ix, "range search");
  });
}

int alaya_index_range_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t ef, const float *d_radii,
                                    uint32_t max_results, const uint32_t *d_allow_words, uint32_t n_masks,
                                    const uint32_t *d_mask_of_query, uint32_t *d_counts, uint32_t *d_ids, float *d_dists,
                                    uint32_t *d_counters, void *stream) {
  return range_device_call(ix, d_queries, nq, ef, d_radii, max_results, d_allow_words, n_masks, d_mask_of_query, d_counts,
                           d_ids, d_dists, d_counters, stream, false, 0, nullptr);
}

int alaya_index_range_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t ef, const float *radii,
                             uint32_t max_results, const uint32_t *allow_words, uint32_t n_masks,
                             const uint32_t *mask_of_query, uint32_t *counts, uint32_t *ids, float *dists,
                             uint32_t *counters) {
  return range_host_call(ix, queries, nq, ef, radii, max_results, allow_words, n_masks, mask_of_query, counts, ids, dists,
                         counters, false, 0, nullptr);
}

int alaya_index_range_search_radius_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t ef,
                                           const float *d_radii, uint32_t max_results, const uint32_t *d_allow_words,
                                           uint32_t n_masks, const uint32_t *d_mask_of_query, uint32_t *d_counts,
                                           uint32_t *d_ids, float *d_dists, uint32_t *d_counters, void *stream,
                                           uint32_t max_frontier, uint32_t *d_more) {
  return range_device_call(ix, d_queries, nq, ef, d_radii, max_results, d_allow_words, n_masks, d_mask_of_query, d_counts,
                           d_ids, d_dists, d_counters, stream, true, max_frontier, d_more);
}

int alaya_index_range_search_radius(alaya_index *ix, const float *queries, uint64_t nq, uint32_t ef, const float *radii,
                                    uint32_t max_results, const uint32_t *allow_words, uint32_t n_masks,
                                    const uint32_t *mask_of_query, uint32_t *counts, uint32_t *ids, float *dists,
                                    uint32_t *counters, uint32_t max_frontier, uint32_t *more) {
  return range_host_call(ix, queries, nq, ef, radii, max_results, allow_words, n_masks, mask_of_query, counts, ids, dists,
                         counters, true, max_frontier, more);
}

// alaya_index_range_search_sq8_device / alaya_index_range_search_sq8: the search stage (do_filtered_search's range plan
// on the SQ8 space) appends the candidates within the code radii to the index's append buffers and counts them in
// d_cand; the rerank measures the stored ones on the f32 rows against d_rq, pads the ones past the exact radius and
// adds the hits to d_counts (zeroed here, on the stream); the sort orders them into d_ids / d_dists.  The caller
// holds ix->mu.
static void range_sq8_dev(alaya_index *ix, const float *d_q, const float *d_rq, uint64_t nq, uint32_t ef,
                          const float *d_radii, const float *d_code_radii, uint32_t max_results, const uint32_t *d_allow,
                          const uint32_t *d_mask_of_query, uint32_t *d_counts, uint32_t *d_cand, uint32_t *d_ids,
                          float *d_dists, uint32_t *d_cnt, hipStream_t s) {
  if (!ix->has_sq8) throw ArgError("index has no SQ8 codes");
  check_range_cap(max_results);
  if (ef == 0) throw ArgError("ef must be >= 1");
  const size_t slots = static_cast<size_t>(nq) * max_results;
  ix->range_ids.reserve(slots * 4);
  ix->range_d.reserve(slots * 4);
  alaya_amd::RangeParams r{};
  r.radii = d_code_radii;
  r.cap = max_results;
  r.append_ids = ix->range_ids.as<uint32_t>();
  r.append_dists = ix->range_d.as<float>();
  r.counts = d_cand;
  r.out_ids = d_ids;
  r.out_dists = d_dists;
  do_filtered_search(ix, d_q, nq, 0, ef, d_allow, d_mask_of_query, nullptr, nullptr, d_cnt, s, true, false, nullptr, &r);
  if (nq == 0) return;
  hip_check(hipMemsetAsync(d_counts, 0, nq * 4, s), "hipMemsetAsync");
  // diagnostics (ALAYA_RANGE_SORT, include/alaya_hip.h), to time the stages: 0 = the search stage alone, counts stay
  // zero; 2 = the search and the rerank without the sort; ids / dists are then left unwritten
  const char *stages = std::getenv("ALAYA_RANGE_SORT");
  if (stages && std::atoi(stages) == 0) return;
  SearchParams p = base_params(ix);
  p.queries = d_rq ? d_rq : d_q;
  p.nq = nq;
  p.q_stride = ix->dim;
  r.radii = d_radii;
  hip_check(alaya_amd::launch_range_rerank(p, r, d_counts, s), "range rerank launch");
  if (!(stages && std::atoi(stages) == 2)) hip_check(alaya_amd::launch_range_sort(r, nq, s), "range sort launch");
  scratch_release(ix, s);  // the rerank and the sort read the append buffers
}

int alaya_index_range_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries, uint64_t nq,
                                        uint32_t ef, const float *d_radii, const float *d_code_radii, uint32_t max_results,
                                        const uint32_t *d_allow_words, uint32_t n_masks, const uint32_t *d_mask_of_query,
                                        uint32_t *d_counts, uint32_t *d_cand, uint32_t *d_ids, float *d_dists,
                                        uint32_t *d_counters, void *stream) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_radii || !d_code_radii || !d_counts || !d_cand || !d_ids || !d_dists)))
      throw ArgError("invalid arguments");
    check_range_masks(nq, d_allow_words, n_masks, d_mask_of_query, false);
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    range_sq8_dev(ix, d_queries, d_rerank_queries, nq, ef, d_radii, d_code_radii, max_results, d_allow_words,
                  d_mask_of_query, d_counts, d_cand, d_ids, d_dists, d_counters, static_cast<hipStream_t>(stream));
  });
}

int alaya_index_range_search_sq8(alaya_index *ix, const float *queries, const float *rerank_queries, uint64_t nq, uint32_t ef,
                                 const float *radii, const float *code_radii, uint32_t max_results,
                                 const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                 uint32_t *counts, uint32_t *cand, uint32_t *ids, float *dists, uint32_t *counters) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!queries || !radii || !code_radii || !counts || !cand || !ids || !dists)))
      throw ArgError("invalid arguments");
    check_range_masks(nq, allow_words, n_masks, mask_of_query, true);
    for (uint64_t i = 0; i < nq; ++i)
      if (radii[i] != radii[i] || code_radii[i] != code_radii[i]) throw ArgError("range search: a radius is NaN");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    check_range_cap(max_results);  // (before the result buffers are sized by it)
    if (nq == 0) {
      range_sq8_dev(ix, nullptr, nullptr, 0, ef, nullptr, nullptr, max_results, nullptr, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, ix->stream);  // the index's own refusals
      return;
    }
    const float *d_q = stage_queries(ix, queries, nq, max_results);
    const float *d_rq = stage_rerank_queries(ix, rerank_queries, queries, nq);
    const uint32_t *d_allow = allow_words ? stage_masks(ix, allow_words, n_masks) : nullptr;
    const uint32_t *d_groups = allow_words ? stage_mask_indices(ix, mask_of_query, nq) : nullptr;
    ix->range_radii.reserve(nq * 4);
    ix->range_cradii.reserve(nq * 4);
    ix->range_cnt.reserve(nq * 4);
    ix->range_cand.reserve(nq * 4);
    hip_check(hipMemcpyAsync(ix->range_radii.ptr, radii, nq * 4, hipMemcpyHostToDevice, ix->stream), "upload radii");
    hip_check(hipMemcpyAsync(ix->range_cradii.ptr, code_radii, nq * 4, hipMemcpyHostToDevice, ix->stream), "upload radii");
    range_sq8_dev(ix, d_q, d_rq, nq, ef, ix->range_radii.as<float>(), ix->range_cradii.as<float>(), max_results, d_allow,
                  d_groups, ix->range_cnt.as<uint32_t>(), ix->range_cand.as<uint32_t>(), ix->id_buf.as<uint32_t>(),
                  ix->dist_buf.as<float>(), ix->cnt_buf.as<uint32_t>(), ix->stream);
    fetch_results(ix, nq, max_results, ids, dists, counters);
    hip_check(hipMemcpyAsync(counts, ix->range_cnt.ptr, nq * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
    hip_check(hipMemcpyAsync(cand, ix->range_cand.ptr, nq * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
    stream_sync(ix, "range sq8 search");
  });
}

int alaya_index_profile_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                               uint32_t ef, int space, uint32_t *ids, uint32_t *counters, uint64_t *stamps) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!queries || !ids || !stamps))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (nq == 0 || k == 0) return;
    DevBuf st;
    st.reserve(nq * 64);
    hip_check(hipMemsetAsync(st.ptr, 0, nq * 64, ix->stream), "memset");
    const float *d_q = stage_queries(ix, queries, nq, k, "H2D", /*dists=*/false);
    do_search(ix, d_q, nq, k, ef, ix->id_buf.as<uint32_t>(), nullptr, ix->cnt_buf.as<uint32_t>(), ix->stream,
              st.as<uint64_t>(), space == 1);
    fetch_results(ix, nq, k, ids, nullptr, counters);
    hip_check(hipMemcpyAsync(stamps, st.ptr, nq * 64, hipMemcpyDeviceToHost, ix->stream), "D2H");
    stream_sync(ix, "profile search");
  });
}

int alaya_index_distances(alaya_index *ix, const float *queries, uint64_t nq, const uint32_t *ids,
                          uint32_t n, float *out) {
  return guarded([&] {
    if (!ix || (nq && (!queries || !out)) || (n && !ids)) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (!ix->base.ptr) throw ArgError("index has no base vectors");
    if (nq == 0 || n == 0) return;
    if (nq > 65535) throw ArgError("at most 65535 queries per call");
    for (uint32_t i = 0; i < n; ++i)
      if (ids[i] >= ix->n) throw ArgError("id out of range");
    ix->q_buf.reserve(nq * ix->dim * 4);
    ix->dlist_buf.reserve(static_cast<size_t>(n) * 4);
    ix->dout_buf.reserve(nq * n * 4);
    hip_check(hipMemcpyAsync(ix->q_buf.ptr, queries, nq * ix->dim * 4, hipMemcpyHostToDevice, ix->stream), "H2D");
    hip_check(hipMemcpyAsync(ix->dlist_buf.ptr, ids, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, ix->stream), "H2D");
    SearchParams p = base_params(ix);
    p.queries = ix->q_buf.as<float>();
    p.q_stride = ix->dim;
    hip_check(alaya_amd::launch_row_distances(p, ix->dlist_buf.as<uint32_t>(), n,
                                              static_cast<uint32_t>(nq), ix->dout_buf.as<float>(),
                                              ix->stream), "distance launch");
    hip_check(hipMemcpyAsync(out, ix->dout_buf.ptr, nq * n * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
    hip_check(hipStreamSynchronize(ix->stream), "distances");
  });
}

// ---- SQ8 (space/quant/sq8.hpp:78-143, space/sq8_space.hpp) --------------------------------
int alaya_sq8_train(const float *data, uint64_t n, uint32_t dim, float *min_v, float *max_v) {
  return guarded([&] {
    if ((n && !data) || !min_v || !max_v || dim == 0) throw ArgError("invalid arguments");
    for (uint32_t j = 0; j < dim; ++j) {  // SQ8Quantizer ctor: min = max(), max = lowest()
      min_v[j] = std::numeric_limits<float>::max();
      max_v[j] = std::numeric_limits<float>::lowest();
    }
    for (uint64_t i = 0; i < n; ++i) {
      const float *r = data + i * dim;
      for (uint32_t j = 0; j < dim; ++j) {
        if (r[j] < min_v[j]) min_v[j] = r[j];
        if (r[j] > max_v[j]) max_v[j] = r[j];
      }
    }
  });
}

int alaya_sq8_encode(const float *data, uint64_t n, uint32_t dim, const float *min_v,
                     const float *max_v, uint8_t *codes, uint32_t num_threads) {
  return guarded([&] {
    if ((n && (!data || !codes)) || !min_v || !max_v) throw ArgError("invalid arguments");
    auto work = [&](uint64_t lo, uint64_t hi) {
      for (uint64_t i = lo; i < hi; ++i) {
        for (uint32_t j = 0; j < dim; ++j) {  // SQ8Quantizer::quantize (sq8.hpp:118-130)
          const float v = data[i * dim + j], mn = min_v[j], mx = max_v[j];
          uint8_t c;
          if (mx == mn) c = 0;
          else if (v >= mx) c = 255;
          else if (v <= mn) c = 0;
          else c = static_cast<uint8_t>(((v - mn) / (mx - mn)) * 255);
          codes[i * dim + j] = c;
        }
      }
    };
    const uint32_t nt = std::max(1u, std::min<uint32_t>(num_threads, 64));
    std::vector<std::thread> ts;
    const uint64_t per = (n + nt - 1) / nt;
    for (uint32_t t = 0; t < nt; ++t) {
      const uint64_t lo = t * per, hi = std::min(n, lo + per);
      if (lo < hi) ts.emplace_back(work, lo, hi);
    }
    for (auto &t : ts) t.join();
  });
}

int alaya_index_set_sq8(alaya_index *ix, const uint8_t *codes, uint64_t n, uint32_t dim,
                        const float *min_v, const float *max_v, int order) {
  return guarded([&] {
    if (!ix || (n && !codes) || !min_v || !max_v) throw ArgError("invalid arguments");
    if (order != 1 && order != 2) throw ArgError("SQ8 order must be 1 (AVX2) or 2 (AVX-512)");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (ix->base.ptr && (dim != ix->dim || n != ix->n)) throw ArgError("SQ8 codes do not match the base rows");
    scratch_drain(ix);
    const uint32_t cs = (dim + 63) / 64 * 64;
    ix->codes.release();
    ix->codes.reserve(std::max<uint64_t>(n, 1) * cs);
    if (n) {
      hip_check(hipMemsetAsync(ix->codes.ptr, 0, n * cs, ix->stream), "memset");
      hip_check(hipMemcpy2DAsync(ix->codes.ptr, cs, codes, dim, dim, n, hipMemcpyHostToDevice, ix->stream),
                "upload codes");
    }
    ix->sq_min.release();
    ix->sq_max.release();
    ix->sq_min.reserve(dim * 4);
    ix->sq_max.reserve(dim * 4);
    hip_check(hipMemcpyAsync(ix->sq_min.ptr, min_v, dim * 4, hipMemcpyHostToDevice, ix->stream), "upload");
    hip_check(hipMemcpyAsync(ix->sq_max.ptr, max_v, dim * 4, hipMemcpyHostToDevice, ix->stream), "upload");
    hip_check(hipStreamSynchronize(ix->stream), "sync");
    ix->code_stride = cs;
    ix->sq8_order = order;
    ix->has_sq8 = true;
  });
}

// SQ8 graph search (+ optional rerank) on device buffers.  The search writes its ks = k (reference
// rerank) or ef (corrected rerank) ids into ix->sq_ids; the rerank reads them and writes d_ids.
// shard >= 0: shard mode (alaya_index_shard_search_sq8_device) with the reference rerank, the id-0
// zero entries only when shard == 1 (this shard holds global row 0), empty slots (kEmpty, FLT_MAX).
static void sq8_search_dev(alaya_index *ix, const float *d_q, const float *d_rq, uint64_t nq, uint32_t k,
                           uint32_t ef, int rerank, uint32_t *d_ids, float *d_dists, uint32_t *d_cnt,
                           hipStream_t s, int shard = -1) {
  if (rerank < 0 || rerank > 2) throw ArgError("rerank must be 0 (none), 1 (reference) or 2 (corrected)");
  if (nq == 0 || k == 0) return;
  if (!rerank) {
    do_search(ix, d_q, nq, k, ef, d_ids, d_dists, d_cnt, s, nullptr, true, shard >= 0 ? 0xffffffffu : 0u);
    return;
  }
  const bool corrected = rerank == 2;
  const uint32_t ks = corrected ? ef : k;  // corrected: the whole ef pool, kEmpty past the pool
  ix->sq_ids.reserve(nq * ks * 4);
  ix->sq_d.reserve(nq * ks * 4);
  // search fill: the reference's zero-initialised pool slots (rescored as row 0) on a single index
  // and on the shard holding global row 0; empty elsewhere (skipped by the rerank)
  const uint32_t search_fill = (corrected || shard == 0) ? 0xffffffffu : 0u;
  do_search(ix, d_q, nq, ks, ef, ix->sq_ids.as<uint32_t>(), ix->sq_d.as<float>(), d_cnt, s, nullptr, true,
            search_fill);
  alaya_amd::RerankParams r{};
  r.k = k;
  r.n_src = ks;
  r.n_take = corrected ? ef : std::min(k, ef);
  r.zeros = (!corrected && shard != 0 && ef > k) ? ef - k : 0u;
  r.fill_id = shard >= 0 ? 0xffffffffu : 0u;
  rerank_sq_ids(ix, d_rq ? d_rq : d_q, nq, r, d_ids, d_dists, s);
}

int alaya_index_batch_search_sq8(alaya_index *ix, const float *queries, const float *rerank_queries,
                                 uint64_t nq, uint32_t k, uint32_t ef, int rerank, uint32_t *ids,
                                 float *dists, uint32_t *counters) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!queries || !ids))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (nq == 0 || k == 0) return;
    const float *d_q = stage_queries(ix, queries, nq, k, "H2D");
    // without a rerank nothing reads the second query form: not uploaded (the filtered call always uploads it)
    const float *d_rq = rerank ? stage_rerank_queries(ix, rerank_queries, queries, nq, "H2D") : nullptr;
    sq8_search_dev(ix, d_q, d_rq, nq, k, ef, rerank, ix->id_buf.as<uint32_t>(), ix->dist_buf.as<float>(),
                   ix->cnt_buf.as<uint32_t>(), ix->stream);
    fetch_results(ix, nq, k, ids, dists, counters);
    stream_sync(ix, "sq8 search");
  });
}

int alaya_index_batch_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries,
                                        uint64_t nq, uint32_t k, uint32_t ef, int rerank, uint32_t *d_ids,
                                        float *d_dists, uint32_t *d_counters, void *stream) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_ids))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    sq8_search_dev(ix, d_queries, d_rerank_queries, nq, k, ef, rerank, d_ids, d_dists, d_counters,
                   static_cast<hipStream_t>(stream));
  });
}

int alaya_index_shard_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries,
                                        uint64_t nq, uint32_t k, uint32_t ef, int holds_row0, uint32_t *d_ids,
                                        float *d_dists, uint32_t *d_counters, void *stream) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_ids || !d_dists))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    sq8_search_dev(ix, d_queries, d_rerank_queries, nq, k, ef, 1, d_ids, d_dists, d_counters,
                   static_cast<hipStream_t>(stream), holds_row0 ? 1 : 0);
  });
}

// Filtered SQ8 search on device buffers: the search stage leaves every query's candidate pool (m ids by code
// distance, kEmpty past the pool) in ix->sq_ids; the rerank rescores those rows on the f32 base against d_rq and
// writes the first k under (exact distance, id), empty slots (kEmpty, FLT_MAX).  No id-0 entries, no zero fill.
static void filtered_sq8_dev(alaya_index *ix, const float *d_q, const float *d_rq, uint64_t nq, uint32_t k, uint32_t ef,
                             uint32_t pool, const uint32_t *d_allow, const uint32_t *d_mask_of_query, uint32_t *d_ids,
                             float *d_dists, uint32_t *d_cnt, hipStream_t s) {
  if (!ix->has_sq8) throw ArgError("index has no SQ8 codes");
  if (ef == 0) throw ArgError("ef must be >= 1");
  if (k == 0 || k > 224) throw ArgError("filtered search: k must be in 1..224");
  const uint32_t m = pool ? pool : std::min<uint32_t>(224, std::max(k, ef));  // default: the whole traversal pool
  if (m > 224) throw ArgError("filtered search: pool must be in 1..224");
  if (m < k) throw ArgError("filtered search: pool must be at least k");
  if (nq == 0) return;
  ix->sq_ids.reserve(nq * m * 4);
  ix->sq_d.reserve(nq * m * 4);
  do_filtered_search(ix, d_q, nq, m, ef, d_allow, d_mask_of_query, ix->sq_ids.as<uint32_t>(), ix->sq_d.as<float>(), d_cnt, s,
                     true);
  // diagnostics (ALAYA_FILTER_RERANK=0, include/alaya_hip.h): the search stage alone, to time it; ids / dists
  // are then not written
  if (const char *e = std::getenv("ALAYA_FILTER_RERANK"))
    if (std::atoi(e) == 0) return;
  alaya_amd::RerankParams r{};
  r.k = k;
  r.n_src = m;
  r.n_take = m;
  r.zeros = 0u;
  r.fill_id = 0xffffffffu;
  rerank_sq_ids(ix, d_rq ? d_rq : d_q, nq, r, d_ids, d_dists, s);
}

int alaya_index_filtered_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries,
                                           uint64_t nq, uint32_t k, uint32_t ef, uint32_t pool,
                                           const uint32_t *d_allow_words, uint32_t n_masks,
                                           const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists,
                                           uint32_t *d_counters, void *stream) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!d_queries || !d_ids || !d_allow_words))) throw ArgError("invalid arguments");
    check_masks("filtered search", nq, n_masks, d_mask_of_query, false);
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    filtered_sq8_dev(ix, d_queries, d_rerank_queries, nq, k, ef, pool, d_allow_words, d_mask_of_query, d_ids, d_dists,
                     d_counters, static_cast<hipStream_t>(stream));
  });
}

int alaya_index_filtered_search_sq8(alaya_index *ix, const float *queries, const float *rerank_queries, uint64_t nq,
                                    uint32_t k, uint32_t ef, uint32_t pool, const uint32_t *allow_words, uint32_t n_masks,
                                    const uint32_t *mask_of_query, uint32_t *ids, float *dists, uint32_t *counters) {
  return guarded_scratch(ix, [&] {
    if (!ix || (nq && (!queries || !ids || !allow_words))) throw ArgError("invalid arguments");
    check_masks("filtered search", nq, n_masks, mask_of_query, true);
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (k == 0 || k > 224) throw ArgError("filtered search: k must be in 1..224");
    if (nq == 0) return;
    const float *d_q = stage_queries(ix, queries, nq, k);
    const float *d_rq = stage_rerank_queries(ix, rerank_queries, queries, nq);
    const uint32_t *d_allow = stage_masks(ix, allow_words, n_masks);
    const uint32_t *d_groups = stage_mask_indices(ix, mask_of_query, nq);
    filtered_sq8_dev(ix, d_q, d_rq, nq, k, ef, pool, d_allow, d_groups, ix->id_buf.as<uint32_t>(),
                     ix->dist_buf.as<float>(), ix->cnt_buf.as<uint32_t>(), ix->stream);
    fetch_results(ix, nq, k, ids, dists, counters);
    stream_sync(ix, "filtered sq8 search");
  });
}

// ---- flat exact k-NN (MFMA shortlist + exact rescoring) ---------------------------------------
int alaya_index_flat_diag(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k, int ablate,
                          uint32_t *d_ids, float *d_dists, uint32_t *d_flags, uint32_t *d_merge_count,
                          void *stream) {
  return guarded([&] {
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    hipStream_t s = static_cast<hipStream_t>(stream);
    scratch_acquire(ix, s);
    ensure_norms(ix, s);
    int blocks = 0;
    alaya_amd::FlatParams p = flat_params(ix, d_queries, nq, k, d_ids, d_dists, d_flags, &blocks, s);
    flat_prescan(ix, p, s);
    p.ablate = ablate;
    p.merge_count = d_merge_count;
    hip_check(alaya_amd::launch_flat_scan(p, blocks, s), "flat scan");
    scratch_release(ix, s);
  });
}

int alaya_index_flat_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k,
                                   uint32_t *d_ids, float *d_dists, uint32_t *d_flags, void *stream) {
  return guarded([&] {
    if (!ix || (nq && (!d_queries || !d_ids))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (nq == 0) return;
    hipStream_t s = static_cast<hipStream_t>(stream);
    scratch_acquire(ix, s);
    flat_scan_merge(ix, d_queries, nq, k, d_ids, d_dists, d_flags, s);
    scratch_release(ix, s);
  });
}

int alaya_index_flat_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                            uint32_t *ids, float *dists, uint32_t *n_recomputed) {
  return guarded([&] {
    if (!ix || (nq && (!queries || !ids))) throw ArgError("invalid arguments");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (n_recomputed) *n_recomputed = 0;
    if (nq == 0) return;
    scratch_acquire(ix, ix->stream);
    ensure_norms(ix, ix->stream);  // ahead of the upload, where it always ran: flat_scan_merge's own call then returns at once
    const float *d_q = stage_queries(ix, queries, nq, k, "H2D", /*dists=*/true, /*counters=*/false);
    ix->flag_buf.reserve(nq * 4);
    std::vector<uint32_t> flags(nq);
    std::vector<float> dv(nq * k);
    auto run = [&](bool no_single) {
      const alaya_amd::FlatParams p = flat_scan_merge(ix, d_q, nq, k, ix->id_buf.as<uint32_t>(), ix->dist_buf.as<float>(),
                                                      ix->flag_buf.as<uint32_t>(), ix->stream, no_single);
      fetch_results(ix, nq, k, ids, dv.data(), nullptr);
      hip_check(hipMemcpyAsync(flags.data(), ix->flag_buf.ptr, nq * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
      stream_sync(ix, "flat search");
      return p.single;
    };
    if (run(false)) {
      // the single pass's bound is ~8x the split's: on data whose 10th and 32nd distances are that
      // close, more than 1 % of the queries flagged reruns the launch with the bf16 hi/lo split
      // before any exhaustive redo
      uint64_t nflag = 0;
      for (uint64_t q = 0; q < nq; ++q) nflag += flags[q] ? 1 : 0;
      if (nflag * 100 > nq) run(true);
    }
    scratch_release(ix, ix->stream);
    // queries whose shortlist bound did not hold: exhaustive exact distances on the device, over
    // the valid rows only (the scan never returns a row cleared in the validity bitmap)
    uint32_t redo = 0;
    std::vector<uint32_t> vbits;
    for (uint64_t q = 0; q < nq; ++q) {
      if (!flags[q]) continue;
      ++redo;
      if (!ix->iota.ptr || ix->iota.bytes < ix->n * 4) {
        std::vector<uint32_t> io(ix->n);
        for (uint64_t i = 0; i < ix->n; ++i) io[i] = static_cast<uint32_t>(i);
        ix->iota.reserve(ix->n * 4);
        hip_check(hipMemcpy(ix->iota.ptr, io.data(), ix->n * 4, hipMemcpyHostToDevice), "H2D");
      }
      if (ix->has_valid && vbits.empty()) {
        vbits.assign((ix->n + 31) / 32, 0u);
        hip_check(hipMemcpy(vbits.data(), ix->valid.ptr, vbits.size() * 4, hipMemcpyDeviceToHost), "D2H");
      }
      ix->dout_buf.reserve(ix->n * 4);
      SearchParams sp = base_params(ix);
      sp.queries = ix->q_buf.as<float>() + q * ix->dim;
      sp.q_stride = ix->dim;
      hip_check(alaya_amd::launch_row_distances(sp, ix->iota.as<uint32_t>(), static_cast<uint32_t>(ix->n), 1,
                                                ix->dout_buf.as<float>(), ix->stream), "exhaustive");
      std::vector<float> all(ix->n);
      hip_check(hipMemcpyAsync(all.data(), ix->dout_buf.ptr, ix->n * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
      hip_check(hipStreamSynchronize(ix->stream), "exhaustive");
      std::vector<uint32_t> order;
      order.reserve(ix->n);
      for (uint64_t i = 0; i < ix->n; ++i)
        if (vbits.empty() || ((vbits[i >> 5] >> (i & 31)) & 1u)) order.push_back(static_cast<uint32_t>(i));
      const uint64_t kk = std::min<uint64_t>(k, order.size());
      std::partial_sort(order.begin(), order.begin() + kk, order.end(), [&](uint32_t a, uint32_t b) {
        return all[a] < all[b] || (all[a] == all[b] && a < b);
      });
      for (uint64_t j = 0; j < k; ++j) {  // slots past the valid rows: (0xffffffff, FLT_MAX), as the scan
        ids[q * k + j] = j < kk ? order[j] : 0xffffffffu;
        dv[q * k + j] = j < kk ? all[order[j]] : FLT_MAX;
      }
    }
    if (dists) std::memcpy(dists, dv.data(), nq * k * 4);
    if (n_recomputed) *n_recomputed = redo;
  });
}

int alaya_index_flat_last_contraction(const alaya_index *ix, int *contraction) {
  return guarded([&] {
    if (!ix || !contraction) throw ArgError("invalid arguments");
    *contraction = ix->flat_contraction;
  });
}

// ---- exact filtered k-NN: compaction, row-reusing f32 scan, merge (flat_filtered_kernels.hip) ------
static uint64_t env_u64(const char *name) {
  const char *e = std::getenv(name);
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 ? static_cast<uint64_t>(v) : 0;
}
static uint64_t flat_filter_forced_rows() { return env_u64("ALAYA_FLAT_FILTER_CHUNK_ROWS"); }

// ---- what the two exact scans' drivers share (do_flat_filtered, do_flat_range) --------------------------
// Both run between scratch_acquire and scratch_release: the buffers below are the index's scratch.
//
// The queries of each of n_lists id lists as an index list, so outputs land in the caller's order: the queries
// of list g are order[first[g] .. first[g + 1]), and with more than one list `order` is uploaded to ff_qlist
// (the host waits for it).  h_groups: the queries' list indices on the host (checked by the caller), or null:
// with more than one list they are read back from d_groups and checked here.  what: the caller's label.
static std::vector<uint64_t> flat_group_queries(alaya_index *ix, uint64_t nq, uint32_t n_lists, const uint32_t *h_groups,
                                                const uint32_t *d_groups, const char *what, hipStream_t stream) {
  std::vector<uint64_t> first(static_cast<size_t>(n_lists) + 1, 0);
  if (n_lists <= 1) {
    first[n_lists] = nq;
    return first;
  }
  std::vector<uint32_t> groups_read;
  if (!h_groups) {
    groups_read.resize(nq);
    hip_check(hipMemcpyAsync(groups_read.data(), d_groups, nq * 4, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), what);
    check_mask_indices(what, groups_read.data(), nq, n_lists);
    h_groups = groups_read.data();
  }
  for (uint64_t i = 0; i < nq; ++i) ++first[h_groups[i] + 1];
  for (uint32_t g = 0; g < n_lists; ++g) first[g + 1] += first[g];
  std::vector<uint32_t> order(nq);
  std::vector<uint64_t> at(first.begin(), first.end() - 1);
  for (uint64_t i = 0; i < nq; ++i) order[at[h_groups[i]]++] = static_cast<uint32_t>(i);
  ix->ff_qlist.reserve(nq * 4);
  hip_check(hipMemcpyAsync(ix->ff_qlist.ptr, order.data(), nq * 4, hipMemcpyHostToDevice, stream), "upload query lists");
  hip_check(hipStreamSynchronize(stream), what);  // `order` is pageable host memory
  return first;
}

// (words AND valid AND below n) as an ascending id list in ff_ids; returns its length, which the host waits
// for.  what: the caller's label, "flat filtered compaction" or "flat range compaction".  Called once per
// mask: the reserves are of the same sizes each time, so only the first of a call can allocate.
static uint32_t flat_compact_ids(alaya_index *ix, const uint32_t *words, const uint32_t *valid, const char *what,
                                 hipStream_t stream) {
  ix->ff_ids.reserve(std::max<uint64_t>(ix->n, 1) * 4);
  ix->ff_sums.reserve((alaya_amd::flat_filtered_blocks(ix->n) + 1) * 4);
  ix->ff_count.reserve(4);
  hip_check(alaya_amd::launch_flat_filtered_compact(words, valid, ix->n, ix->ff_sums.as<uint32_t>(),
                                                    ix->ff_ids.as<uint32_t>(), ix->ff_count.as<uint32_t>(), stream),
            what);
  uint32_t m = 0;
  hip_check(hipMemcpyAsync(&m, ix->ff_count.ptr, 4, hipMemcpyDeviceToHost, stream), "D2H");
  hip_check(hipStreamSynchronize(stream), what);
  if (m > ix->n) throw DeviceError(std::string(what) + ": count past the rows");
  return m;
}

// Every pointer but h_groups is a device pointer.  h_groups: the queries' mask indices on the host (checked
// by the caller), or null: with more than one mask they are read back from d_groups and checked.
// Masks are served one after another on `stream`; the host waits for each mask's allowed-row count.
static void do_flat_filtered(alaya_index *ix, const float *d_q, uint64_t nq, uint32_t k, const uint32_t *d_allow,
                             uint32_t n_masks, const uint32_t *h_groups, const uint32_t *d_groups, uint32_t *d_ids,
                             float *d_dists, hipStream_t stream) {
  using namespace alaya_amd;
  if (!ix->base.ptr) throw ArgError("index has no base vectors");
  if (ix->generic) throw ArgError("flat filtered search: float32 rows only");
  if (k == 0 || k > kFilteredMaxK) throw ArgError("flat filtered search: k must be in 1..224");
  if (nq == 0) return;
  if (nq > 0xffffffffull) throw ArgError("flat filtered search: too many queries");
  const uint64_t mask_words = (ix->n + 31) / 32;
  const uint64_t forced = flat_filter_forced_rows();
  const uint32_t cus = static_cast<uint32_t>(stream_cus(ix, stream));
  scratch_acquire(ix, stream);
  const std::vector<uint64_t> first = flat_group_queries(ix, nq, n_masks, h_groups, d_groups, "flat filtered search", stream);
  uint64_t stats[4] = {0, 0, 0, 0};
  for (uint32_t g = 0; g < n_masks; ++g) {
    const uint64_t nq_g = first[g + 1] - first[g];
    if (nq_g == 0) continue;
    const uint32_t m = flat_compact_ids(ix, d_allow + static_cast<uint64_t>(g) * mask_words,
                                        ix->has_valid ? ix->valid.as<uint32_t>() : nullptr, "flat filtered compaction", stream);
    const FlatFilteredPlan plan = flat_filtered_plan(m, nq_g, k, ix->stride, cus, forced);
    if (plan.tile == 0) throw ArgError("flat filtered search: k / dim too large for the LDS budget");
    stats[0] += m;
    FlatFilteredParams p{};
    p.base = ix->base.as<float>();
    p.dim = ix->dim;
    p.stride = ix->stride;
    p.ip = ix->metric == ALAYA_METRIC_L2 ? 0 : 1;
    p.queries = d_q;
    p.q_stride = ix->dim;
    p.q_list = n_masks > 1 ? ix->ff_qlist.as<uint32_t>() : nullptr;
    p.ids = ix->ff_ids.as<uint32_t>();
    p.n_ids = m;
    p.chunk_rows = plan.chunk_rows;
    p.chunks = plan.chunks;
    p.tile = static_cast<uint32_t>(plan.tile);
    p.k = k;
    p.out_ids = d_ids;
    p.out_dists = d_dists;
    if (m) {
      // (a buffer that grows is freed first, which waits for the launches that still read it)
      ix->ff_part_d.reserve(plan.partial_bytes / 2);
      ix->ff_part_i.reserve(plan.partial_bytes / 2);
      p.part_d = ix->ff_part_d.as<float>();
      p.part_i = ix->ff_part_i.as<uint32_t>();
    }
    for (uint64_t sb = 0; sb < nq_g; sb += plan.sub_queries) {
      p.q_first = first[g] + sb;
      p.nq = std::min<uint64_t>(plan.sub_queries, nq_g - sb);
      if (m) {
        hip_check(launch_flat_filtered_scan(p, stream), "flat filtered scan");
        stats[1] = plan.chunks;
        stats[2] = plan.tile;
        ++stats[3];
      }
      hip_check(launch_flat_filtered_merge(p, stream), "flat filtered merge");  // m = 0: empty slots
    }
  }
  scratch_release(ix, stream);
  std::memcpy(ix->ff_last, stats, sizeof(stats));
}

int alaya_index_flat_search_filtered_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k,
                                            const uint32_t *d_allow_words, uint32_t n_masks,
                                            const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists,
                                            void *stream) {
  return guarded([&] {
    if (!ix || (nq && (!d_queries || !d_ids || !d_allow_words))) throw ArgError("invalid arguments");
    check_masks("flat filtered search", nq, n_masks, d_mask_of_query, false);  // (do_flat_filtered reads them back)
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    do_flat_filtered(ix, d_queries, nq, k, d_allow_words, n_masks, nullptr, d_mask_of_query, d_ids, d_dists,
                     static_cast<hipStream_t>(stream));
  });
}

int alaya_index_flat_search_filtered(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                                     const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                     uint32_t *ids, float *dists) {
  return guarded([&] {
    if (!ix || (nq && (!queries || !ids || !allow_words))) throw ArgError("invalid arguments");
    check_masks("flat filtered search", nq, n_masks, mask_of_query, true);
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    if (k == 0 || k > 224) throw ArgError("flat filtered search: k must be in 1..224");
    if (nq == 0) return;
    scratch_acquire(ix, ix->stream);  // the upload buffers below are the index's, shared with other launches
    const float *d_q = stage_queries(ix, queries, nq, k, "upload queries", /*dists=*/true, /*counters=*/false);
    const uint32_t *d_allow = stage_masks(ix, allow_words, n_masks);
    // the scan orders the queries by mask on the host: it takes the host's indices (no group_buf), and only
    // where there is more than one mask to order by
    do_flat_filtered(ix, d_q, nq, k, d_allow, n_masks, n_masks > 1 ? mask_of_query : nullptr, nullptr,
                     ix->id_buf.as<uint32_t>(), ix->dist_buf.as<float>(), ix->stream);
    fetch_results(ix, nq, k, ids, dists, nullptr);
    stream_sync(ix, "flat filtered search");
  });
}

int alaya_index_flat_filtered_last(const alaya_index *ix, uint64_t *out) {
  return guarded([&] {
    if (!ix || !out) throw ArgError("invalid arguments");
    std::memcpy(out, ix->ff_last, sizeof(ix->ff_last));
  });
}

int alaya_flat_filtered_plan(uint64_t n_allowed, uint64_t nq, uint32_t k, uint32_t stride, uint32_t cus,
                             uint64_t *out) {
  return guarded([&] {
    if (!out) throw ArgError("invalid arguments");
    if (k == 0 || k > alaya_amd::kFilteredMaxK) throw ArgError("flat filtered plan: k must be in 1..224");
    const alaya_amd::FlatFilteredPlan r = alaya_amd::flat_filtered_plan(n_allowed, nq, k, stride, cus, flat_filter_forced_rows());
    if (r.tile == 0) throw ArgError("flat filtered plan: k / dim too large for the LDS budget");
    out[0] = r.chunk_rows;
    out[1] = r.chunks;
    out[2] = r.tile;
    out[3] = r.sub_queries;
    out[4] = r.partial_bytes;
  });
}

// ---- exact range search: compaction, row-reusing f32 scan with a threshold, gather, sort (flat_range_kernels.hip) ----
static uint64_t flat_range_forced_rows() { return env_u64("ALAYA_FLAT_RANGE_CHUNK_ROWS"); }
static uint64_t flat_range_forced_staging() { return env_u64("ALAYA_FLAT_RANGE_STAGING_BYTES"); }

// Every pointer but h_groups is a device pointer.  d_allow null (n_masks 0): no mask.  h_groups / d_groups as
// do_flat_filtered's.  Masks are served one after another on `stream`; the host waits for each mask's
// eligible-row count, never for the radii.
static void do_flat_range(alaya_index *ix, const float *d_q, uint64_t nq, const float *d_radii, uint32_t max_results,
                          const uint32_t *d_allow, uint32_t n_masks, const uint32_t *h_groups, const uint32_t *d_groups,
                          uint32_t *d_counts, uint32_t *d_ids, float *d_dists, hipStream_t stream) {
  using namespace alaya_amd;
  if (!ix->base.ptr) throw ArgError("index has no base vectors");
  if (ix->generic) throw ArgError("flat range search: float32 rows only");
  if (max_results == 0 || max_results > kFlatRangeMaxCap) throw ArgError("flat range search: max_results must be in 1..4096");
  if (nq == 0) return;
  if (nq > 0xffffffffull) throw ArgError("flat range search: too many queries");
  const bool masked = d_allow != nullptr;
  const uint32_t n_lists = masked ? n_masks : 1;  // id lists to scan: one per mask, or the one of no mask
  const uint64_t mask_words = (ix->n + 31) / 32;
  const uint64_t forced = flat_range_forced_rows(), forced_staging = flat_range_forced_staging();
  const uint32_t cus = static_cast<uint32_t>(stream_cus(ix, stream));
  const char *stages_env = std::getenv("ALAYA_FLAT_RANGE_STAGES");
  const int stages = stages_env ? std::atoi(stages_env) : 3;  // diagnostics: 1 = scans only, 2 = and gathers, else all
  scratch_acquire(ix, stream);
  const std::vector<uint64_t> first = flat_group_queries(ix, nq, n_lists, h_groups, d_groups, "flat range search", stream);
  const uint32_t *d_valid = ix->has_valid ? ix->valid.as<uint32_t>() : nullptr;
  if (!masked && !d_valid) {  // no mask, every row valid: the compaction runs over all-ones words
    ix->fr_ones.reserve(std::max<uint64_t>(mask_words, 1) * 4);
    hip_check(hipMemsetAsync(ix->fr_ones.ptr, 0xff, mask_words * 4, stream), "flat range search");
  }
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t g = 0; g < n_lists; ++g) {
    const uint64_t nq_g = first[g + 1] - first[g];
    if (nq_g == 0) continue;
    // (mask AND validity AND below n); with no mask the validity bitmap, or the all-ones words, is the mask
    const uint32_t *words = masked ? d_allow + static_cast<uint64_t>(g) * mask_words
                                   : (d_valid ? d_valid : ix->fr_ones.as<uint32_t>());
    const uint32_t m = flat_compact_ids(ix, words, masked ? d_valid : nullptr, "flat range compaction", stream);
    const FlatRangePlan plan = flat_range_plan(m, nq_g, max_results, ix->stride, cus, forced, forced_staging);
    if (plan.tile == 0) throw ArgError("flat range search: dim too large for the LDS budget");
    stats[0] = m;
    stats[1] = plan.chunks;
    stats[2] = plan.tile;
    stats[3] = 0;
    stats[4] += m;
    FlatRangeParams p{};
    p.base = ix->base.as<float>();
    p.dim = ix->dim;
    p.stride = ix->stride;
    p.ip = ix->metric == ALAYA_METRIC_L2 ? 0 : 1;
    p.queries = d_q;
    p.q_stride = ix->dim;
    p.radii = d_radii;
    p.q_list = n_lists > 1 ? ix->ff_qlist.as<uint32_t>() : nullptr;
    p.ids = ix->ff_ids.as<uint32_t>();
    p.n_ids = m;
    p.chunk_rows = plan.chunk_rows;
    p.chunks = plan.chunks;
    p.tile = static_cast<uint32_t>(plan.tile);
    p.cap = max_results;
    p.slots = static_cast<uint32_t>(plan.slots);
    p.out_counts = d_counts;
    p.out_ids = d_ids;
    p.out_dists = d_dists;
    if (m) {
      // (a buffer that grows is freed first, which waits for the launches that still read it)
      const uint64_t pairs = plan.chunks * std::min<uint64_t>(nq_g, plan.sub_queries);
      ix->ff_part_d.reserve(pairs * plan.slots * 4);
      ix->ff_part_i.reserve(pairs * plan.slots * 4);
      ix->fr_part_n.reserve(pairs * 4);
      p.part_d = ix->ff_part_d.as<float>();
      p.part_i = ix->ff_part_i.as<uint32_t>();
      p.part_n = ix->fr_part_n.as<uint32_t>();
    }
    for (uint64_t sb = 0; sb < nq_g; sb += plan.sub_queries) {
      p.q_first = first[g] + sb;
      p.nq = std::min<uint64_t>(plan.sub_queries, nq_g - sb);
      if (m) {
        hip_check(launch_flat_range_scan(p, stream), "flat range scan");
        ++stats[3];
        ++stats[5];
      }
      if (stages >= 2) hip_check(launch_flat_range_gather(p, stream), "flat range gather");  // m = 0: empty rows
    }
  }
  if (stages >= 3) {
    // the gather left each row's first min(count, cap) hits in id order: range_sort_kernel orders them in place
    // (a workgroup reads its whole row into LDS before it writes any of it)
    RangeParams r{};
    r.radii = d_radii;
    r.cap = max_results;
    r.append_ids = d_ids;
    r.append_dists = d_dists;
    r.counts = d_counts;
    r.out_ids = d_ids;
    r.out_dists = d_dists;
    hip_check(launch_range_sort(r, nq, stream), "flat range sort");
  }
  scratch_release(ix, stream);
  std::memcpy(ix->fr_last, stats, sizeof(stats));
}

int alaya_index_flat_range_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, const float *d_radii,
                                         uint32_t max_results, const uint32_t *d_allow_words, uint32_t n_masks,
                                         const uint32_t *d_mask_of_query, uint32_t *d_counts, uint32_t *d_ids,
                                         float *d_dists, void *stream) {
  return guarded([&] {
    if (!ix || (nq && (!d_queries || !d_radii || !d_counts || !d_ids || !d_dists))) throw ArgError("invalid arguments");
    check_range_masks(nq, d_allow_words, n_masks, d_mask_of_query, false);  // (do_flat_range reads the indices back)
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    do_flat_range(ix, d_queries, nq, d_radii, max_results, d_allow_words, n_masks, nullptr, d_mask_of_query, d_counts,
                  d_ids, d_dists, static_cast<hipStream_t>(stream));
  });
}

int alaya_index_flat_range_search(alaya_index *ix, const float *queries, uint64_t nq, const float *radii,
                                  uint32_t max_results, const uint32_t *allow_words, uint32_t n_masks,
                                  const uint32_t *mask_of_query, uint32_t *counts, uint32_t *ids, float *dists) {
  return guarded([&] {
    if (!ix || (nq && (!queries || !radii || !counts || !ids || !dists))) throw ArgError("invalid arguments");
    check_range_masks(nq, allow_words, n_masks, mask_of_query, true);
    for (uint64_t i = 0; i < nq; ++i)
      if (radii[i] != radii[i]) throw ArgError("flat range search: a radius is NaN");
    std::lock_guard<std::mutex> lk(ix->mu);
    set_device(ix);
    check_range_cap(max_results);  // (before the result buffers are sized by it)
    if (nq == 0) {
      do_flat_range(ix, nullptr, 0, nullptr, max_results, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                    ix->stream);  // the index's own refusals
      return;
    }
    scratch_acquire(ix, ix->stream);  // the upload buffers below are the index's, shared with other launches
    const float *d_q = stage_queries(ix, queries, nq, max_results, "upload queries", /*dists=*/true, /*counters=*/false);
    const uint32_t *d_allow = allow_words ? stage_masks(ix, allow_words, n_masks) : nullptr;
    ix->range_radii.reserve(nq * 4);
    ix->range_cnt.reserve(nq * 4);
    hip_check(hipMemcpyAsync(ix->range_radii.ptr, radii, nq * 4, hipMemcpyHostToDevice, ix->stream), "upload radii");
    // the scan orders the queries by mask on the host: it takes the host's indices, and only where there is more
    // than one mask to order by
    do_flat_range(ix, d_q, nq, ix->range_radii.as<float>(), max_results, d_allow, n_masks,
                  n_masks > 1 ? mask_of_query : nullptr, nullptr, ix->range_cnt.as<uint32_t>(), ix->id_buf.as<uint32_t>(),
                  ix->dist_buf.as<float>(), ix->stream);
    fetch_results(ix, nq, max_results, ids, dists, nullptr);
    hip_check(hipMemcpyAsync(counts, ix->range_cnt.ptr, nq * 4, hipMemcpyDeviceToHost, ix->stream), "D2H");
    stream_sync(ix, "flat range search");
  });
}

int alaya_index_flat_range_last(const alaya_index *ix, uint64_t *out) {
  return guarded([&] {
    if (!ix || !out) throw ArgError("invalid arguments");
    std::memcpy(out, ix->fr_last, sizeof(ix->fr_last));
  });
}

int alaya_flat_range_plan(uint64_t n_eligible, uint64_t nq, uint32_t max_results, uint32_t stride, uint32_t cus,
                          uint64_t *out) {
  return guarded([&] {
    if (!out) throw ArgError("invalid arguments");
    if (max_results == 0 || max_results > alaya_amd::kFlatRangeMaxCap)
      throw ArgError("flat range plan: max_results must be in 1..4096");
    const alaya_amd::FlatRangePlan r = alaya_amd::flat_range_plan(n_eligible, nq, max_results, stride, cus,
                                                                  flat_range_forced_rows(), flat_range_forced_staging());
    if (r.tile == 0) throw ArgError("flat range plan: dim too large for the LDS budget");
    out[0] = r.chunk_rows;
    out[1] = r.chunks;
    out[2] = r.tile;
    out[3] = r.sub_queries;
    out[4] = r.slots;
    out[5] = r.staging_bytes;
  });
}

int alaya_index_set_hash_log2(alaya_index *ix, uint32_t log2_slots) {
  return guarded([&] {
    if (!ix) throw ArgError("null index");
    if (log2_slots != 0 && (log2_slots < 6 || log2_slots > 16)) throw ArgError("log2_slots must be 0 or 6..16");
    ix->hash_log2_override = log2_slots;
  });
}

int alaya_stream_create_reserving(int device, uint32_t reserved_cus, void **stream) {
  return guarded([&] {
    if (!stream) throw ArgError("null stream pointer");
    hip_check(hipSetDevice(device), "hipSetDevice");
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
    const uint32_t n = static_cast<uint32_t>(prop.multiProcessorCount);
    if (reserved_cus >= n) throw ArgError("reserved_cus must leave at least one CU");
    std::vector<uint32_t> mask((n + 31) / 32, 0u);
    for (uint32_t c = 0; c < n; ++c) mask[c / 32] |= 1u << (c % 32);
    // The reserved CUs go one per XCD in turn.  Which XCD a CU-mask bit names is not documented
    // (the bits may interleave, CU i on XCD i mod X, or run in blocks, CU i on XCD i / (n / X)), so
    // reserved CU r is chosen on XCD r mod X under both numberings: c = x * (n / X) + ((x + X k) mod
    // (n / X)) with x = r mod X, k = r / X (c mod X = x when X divides n / X).  A CU already taken
    // (more than n / X reserved) moves to the next free one.
    int xcds = 1;
    if (hipDeviceGetAttribute(&xcds, hipDeviceAttributeNumberOfXccs, device) != hipSuccess || xcds < 1) {
      (void)hipGetLastError();
      xcds = 1;
    }
    const uint32_t X = static_cast<uint32_t>(xcds);
    const uint32_t per = (n % X == 0) ? n / X : n;  // CUs per XCD (1 block when X does not divide n)
    const uint32_t xs = (n % X == 0) ? X : 1u;
    for (uint32_t r = 0; r < reserved_cus; ++r) {
      const uint32_t x = r % xs, k = r / xs;
      uint32_t c = x * per + (x + xs * k) % per;
      while (!(mask[c / 32] & (1u << (c % 32)))) c = (c + 1) % n;  // reserved_cus < n: a free CU exists
      mask[c / 32] &= ~(1u << (c % 32));
    }
    hipStream_t s = nullptr;
    hip_check(hipExtStreamCreateWithCUMask(&s, static_cast<uint32_t>(mask.size()), mask.data()),
              "hipExtStreamCreateWithCUMask");
    *stream = s;
  });
}

int alaya_stream_destroy(void *stream) {
  return guarded([&] {
    if (stream) hip_check(hipStreamDestroy(static_cast<hipStream_t>(stream)), "hipStreamDestroy");
  });
}

int alaya_index_last_launch(const alaya_index *ix, uint32_t *workgroups, uint32_t *waves_per_group) {
  return guarded([&] {
    if (!ix) throw ArgError("null index");
    if (workgroups) *workgroups = ix->last_grid;
    if (waves_per_group) *waves_per_group = ix->last_waves;
  });
}

int alaya_index_last_plan(const alaya_index *ix, uint32_t *lds_bytes, uint32_t *hash_log2, uint32_t *compact,
                          uint32_t *groups_per_cu, uint32_t *scout) {
  return guarded([&] {
    if (!ix) throw ArgError("null index");
    if (lds_bytes) *lds_bytes = ix->last_lds;
    if (hash_log2) *hash_log2 = ix->last_hash_log2;
    if (compact) *compact = ix->last_compact;
    if (groups_per_cu) *groups_per_cu = ix->last_per_cu;
    if (scout) *scout = ix->last_scout;
  });
}

// The sums, per word, of a per-searcher counter buffer of the last search (`words` 32-bit words for
// each of `searchers`): waits for the index's stream, then copies the buffer to the host.
static std::vector<uint64_t> searcher_stats(alaya_index *ix, const DevBuf &buf, uint64_t searchers, uint32_t words) {
  std::vector<uint64_t> t(words, 0);
  if (searchers) {
    set_device(ix);
    scratch_drain(ix);
    std::vector<uint32_t> h(words * searchers);
    hip_check(hipMemcpy(h.data(), buf.ptr, h.size() * 4, hipMemcpyDeviceToHost), "D2H");
    for (uint64_t i = 0; i < h.size(); ++i) t[i % words] += h[i];
  }
  return t;
}

int alaya_index_scout_stats(alaya_index *ix, uint64_t *expansions, uint64_t *hits, uint64_t *records,
                            uint64_t *mismatches) {
  return guarded_scratch(ix, [&] {
    if (!ix) throw ArgError("null index");
    const std::vector<uint64_t> t = searcher_stats(ix, ix->scout_stats, ix->scout_stats_slots, 4);
    if (expansions) *expansions = t[0];
    if (hits) *hits = t[1];
    if (records) *records = t[2];
    if (mismatches) *mismatches = t[3];
  });
}

int alaya_index_scout_policy_stats(alaya_index *ix, uint32_t *policy, uint64_t *early_posts, uint64_t *confirmed,
                                   uint64_t *abandoned) {
  return guarded_scratch(ix, [&] {
    if (!ix) throw ArgError("null index");
    const bool sums = early_posts || confirmed || abandoned;  // (the mask alone: no wait)
    const std::vector<uint64_t> t = searcher_stats(ix, ix->scout_policy_stats, sums ? ix->scout_stats_slots : 0, 3);
    if (policy) *policy = ix->last_scout_policy;
    if (early_posts) *early_posts = t[0];
    if (confirmed) *confirmed = t[1];
    if (abandoned) *abandoned = t[2];
  });
}

int alaya_index_set_helpers(alaya_index *ix, int mode) {
  return guarded([&] {
    if (!ix) throw ArgError("null index");
    if (mode < -1 || mode > 1) throw ArgError("helpers mode must be -1 (automatic), 0 (off) or 1 (on)");
    ix->helpers_mode = mode;
  });
}

int alaya_index_help_stats(alaya_index *ix, uint64_t *memo_dists, uint64_t *memo_expansions, uint64_t *helper_rows) {
  return guarded_scratch(ix, [&] {
    if (!ix) throw ArgError("null index");
    const std::vector<uint64_t> t = searcher_stats(ix, ix->help_stats, ix->help_stats_slots, 3);
    if (memo_dists) *memo_dists = t[0];
    if (memo_expansions) *memo_expansions = t[1];
    if (helper_rows) *helper_rows = t[2];
  });
}

int alaya_screen_lower_bound(const float *d_tilde, const float *e_row, uint64_t n, uint32_t dim, float *out) {
  return guarded([&] {
    if (n && (!d_tilde || !e_row || !out)) throw ArgError("invalid arguments");
    for (uint64_t i = 0; i < n; ++i) out[i] = alaya_amd::screen_lower_bound(d_tilde[i], e_row[i], dim);
  });
}

namespace {
// One vector through the 8-bit screening quantiser, as screen_rows_u8_kernel runs it on a row and
// screen_query_codes on a query: codes, header {err, lo, scale, 0} and, where asked for, the f32
// values the codes stand for.
void screen_u8_quantize_one(const float *x, uint32_t dim, uint8_t *codes, float *header, float *values) {
  using namespace alaya_amd;
  float lo = FLT_MAX, hi = -FLT_MAX;
  bool bad = false;
  for (uint32_t j = 0; j < dim; ++j) {
    bad = bad || !screen_finite(x[j]);
    lo = fminf(lo, x[j]);
    hi = fmaxf(hi, x[j]);
  }
  float scale = screen_u8_scale(lo, hi);
  if (bad || !screen_finite(scale)) {
    bad = true;
    lo = scale = 0.f;
  }
  float sum = 0.f;
  for (uint32_t j = 0; j < dim; ++j) {
    const uint32_t c = screen_u8_code(x[j], lo, scale);
    const float y = screen_u8_value(c, lo, scale);
    const float d = x[j] - y;
    if (!bad) sum = fmaf(d, d, sum);
    codes[j] = static_cast<uint8_t>(c);
    if (values) values[j] = y;
  }
  header[0] = screen_u8_err(sum, dim, bad);
  header[1] = lo;
  header[2] = scale;
  header[3] = 0.f;
}
}  // namespace

int alaya_screen_u8_quantize(const float *rows, uint64_t n, uint32_t dim, uint8_t *codes, float *header,
                             float *values) {
  return guarded([&] {
    if (n && dim && (!rows || !codes || !header || !values)) throw ArgError("invalid arguments");
    for (uint64_t r = 0; r < n; ++r)
      screen_u8_quantize_one(rows + r * dim, dim, codes + r * dim, header + 4 * r, values + r * dim);
  });
}

int alaya_screen_int_bound(const float *queries, const float *rows, uint64_t n, uint32_t dim, float *d_in,
                           float *e_sum, float *bound, uint32_t *sums) {
  return guarded([&] {
    using namespace alaya_amd;
    if (dim == 0 || dim > 4096) throw ArgError("dim must be in 1 .. 4096");
    if (n && (!queries || !rows || !d_in || !e_sum || !bound || !sums)) throw ArgError("invalid arguments");
    std::vector<uint8_t> a(dim), c(dim);
    for (uint64_t i = 0; i < n; ++i) {
      float qh[4], rh[4];
      screen_u8_quantize_one(queries + i * dim, dim, a.data(), qh, nullptr);
      screen_u8_quantize_one(rows + i * dim, dim, c.data(), rh, nullptr);
      uint32_t a1 = 0, a2 = 0, c1 = 0, c2 = 0, ac = 0;
      for (uint32_t j = 0; j < dim; ++j) {
        const uint32_t aj = a[j], cj = c[j];
        a1 += aj; a2 += aj * aj;
        c1 += cj; c2 += cj * cj;
        ac += aj * cj;
      }
      d_in[i] = screen_int_distance(dim, qh[1], qh[2], a1, a2, rh[1], rh[2], c1, c2, ac);
      e_sum[i] = screen_int_err(rh[0], rh[1], rh[2], qh[0], qh[1], qh[2]);
      bound[i] = screen_int_bound(dim, qh[0], qh[1], qh[2], a1, a2, rh[0], rh[1], rh[2], c1, c2, ac);
      uint32_t *s = sums + 5 * i;
      s[0] = a1; s[1] = a2; s[2] = c1; s[3] = c2; s[4] = ac;
    }
  });
}

int alaya_flat_ip_slack(int contraction, uint32_t k_acc, const float *q_norm2, const int *q_exp, uint64_t n,
                        float b_max, int base_exp, float *out) {
  return guarded([&] {
    if (contraction < 0 || contraction > 2 || (n && (!q_norm2 || !out))) throw ArgError("invalid arguments");
    for (uint64_t i = 0; i < n; ++i)
      out[i] = alaya_amd::flat_ip_slack(contraction, k_acc, q_norm2[i], q_exp ? q_exp[i] : 0, b_max, base_exp);
  });
}

int alaya_flat_ip_proven(const float *kth_d, const float *cutoff, const float *slack, uint64_t n, uint8_t *out) {
  return guarded([&] {
    if (n && (!kth_d || !cutoff || !slack || !out)) throw ArgError("invalid arguments");
    for (uint64_t i = 0; i < n; ++i) out[i] = alaya_amd::flat_ip_proven(kth_d[i], cutoff[i], slack[i]) ? 1 : 0;
  });
}

int alaya_search_variant(uint32_t dim, int ip, int sq8_order, int generic, uint32_t wanted_mode, int *space,
                         uint32_t *chunks, uint32_t *mode, uint32_t *has_mode) {
  return guarded([&] {
    using namespace alaya_amd;
    if (sq8_order < 0 || sq8_order > 2 || wanted_mode >= 32u) throw ArgError("invalid arguments");
    const SearchVariant &v = resolve_search_variant({dim, ip != 0, sq8_order, generic != 0, static_cast<int>(wanted_mode)});
    if (space) *space = v.space;
    if (chunks) *chunks = static_cast<uint32_t>(v.chunks);
    if (mode) *mode = static_cast<uint32_t>(v.mode);
    if (has_mode)
      *has_mode = (search_has_helpers(dim, sq8_order, generic != 0) ? kModeHelp : 0) |
                  (search_has_two_waves(dim, sq8_order, generic != 0) ? kModeTwoWaves : 0) |
                  (search_has_screen(dim, sq8_order, generic != 0, ip != 0) ? kModeScreen : 0);
  });
}

int alaya_search_variant_at(uint32_t index, int *space, uint32_t *chunks, uint32_t *mode, int *l2_only,
                            uint32_t *count) {
  return guarded([&] {
    if (count) *count = static_cast<uint32_t>(alaya_amd::kNumSearchVariants);
    if (index >= alaya_amd::kNumSearchVariants) throw ArgError("variant index out of range");
    const alaya_amd::SearchVariant &v = alaya_amd::kSearchVariants[index];
    if (space) *space = v.space;
    if (chunks) *chunks = static_cast<uint32_t>(v.chunks);
    if (mode) *mode = static_cast<uint32_t>(v.mode);
    if (l2_only) *l2_only = v.l2_only ? 1 : 0;
  });
}

int alaya_index_screen_stats(alaya_index *ix, uint64_t *screened, uint64_t *screened_out) {
  return guarded_scratch(ix, [&] {
    if (!ix) throw ArgError("null index");
    const std::vector<uint64_t> t = searcher_stats(ix, ix->screen_stats, ix->screen_stats_slots, 2);
    if (screened) *screened = t[0];
    if (screened_out) *screened_out = t[1];
  });
}

int alaya_index_set_visited_mode(alaya_index *ix, int mode) {
  return guarded([&] {
    if (!ix) throw ArgError("null index");
    if (mode < 0 || mode > 3) throw ArgError("visited mode must be 0 (auto), 1 (compact), 2 (wide) or 3 (test)");
    ix->visited_mode_override = mode;
  });
}

int alaya_index_info(const alaya_index *ix, uint64_t *n, uint32_t *dim, uint32_t *stride,
                     int *metric, uint64_t *device_bytes) {
  return guarded([&] {
    if (!ix) throw ArgError("null index");
    if (n) *n = ix->n;
    if (dim) *dim = ix->dim;
    if (stride) *stride = ix->stride;
    if (metric) *metric = ix->metric;
    if (device_bytes) *device_bytes = ix->device_bytes();
  });
}

}  // extern "C"
