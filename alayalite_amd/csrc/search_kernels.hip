// MI355X (gfx950) device code for the HNSW best-first search hot path.
//
// One wavefront (64 lanes) owns one query at a time; workgroups are single waves that pull query
// indices from a device work counter until the batch is drained (persistent blocks).  Per query:
//   * query vector staged in LDS, zero-padded to the row stride;
//   * the candidate pool (the reference's LinearPool, include/utils/query_utils.hpp:236-312) is a
//     sorted LDS array of (dist, id|checked) with capacity ef;
//   * the visited set (DynamicBitset, query_utils.hpp:69-115) is an exact LDS open-addressing hash
//     table that spills to a per-slot global bitset when it fills;
//   * one expansion = read a 128 B adjacency row, filter visited ids in adjacency order, compute all
//     new distances at once (8 lanes per row, 8 rows per wave pass, 128 B-coalesced row chunks), then
//     merge the batch into the pool with a wave-parallel stable merge that is provably identical to
//     inserting the neighbours one by one (graph_search_job.hpp:237-251 + LinearPool::insert).
// The distance reproduces l2_sqr_avx2 / ip_sqr_avx2 (include/simd/distance_l2.ipp:54-116,
// distance_ip.ipp:56-111) bit for bit: lane m of a row group owns partial sums acc[4m..4m+3]
// (element 32t+j -> acc[j]), the 8-lane combine follows the AVX2 horizontal tree exactly.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "screen_bound.h"
#include "search_kernels.h"
#include "search_device.h"

// Minimum waves per SIMD the compiler must leave room for, per search-kernel shape (the register
// budget: 512 / waves VGPRs).  0 = no constraint.  Diagnostics builds override with
// -DALAYA_MIN_WAVES_SQ8=... / -DALAYA_MIN_WAVES_NARROW=....
#ifndef ALAYA_MIN_WAVES_SQ8
// The AVX-512-order SQ8 kernels (config 5 on an AVX-512 host) are held to 4 waves per SIMD (128
// VGPRs): with the spill table the 768-d IP kernel needs 129 and would drop to 3; at 128 the
// allocator spills one 8-byte value that is live across the whole query loop (a store at kernel
// entry, a load after the loop), nothing per expansion.  The AVX2-order kernels would spill inside
// the expansion loop (32-136 B of scratch) and keep their natural budget.
#define ALAYA_MIN_WAVES_SQ8 -1
#endif
#ifndef ALAYA_MIN_WAVES_NARROW
#define ALAYA_MIN_WAVES_NARROW 0
#endif
#ifndef ALAYA_MIN_WAVES_WIDE
#define ALAYA_MIN_WAVES_WIDE 0  // diagnostics: waves per SIMD for the f32 kernels with d > 256
#endif
// kSpace: 0 = f32 rows, 1 = SQ8 codes in the AVX2 order, 2 = SQ8 codes in the AVX-512 order (the
// kernels that run on the spill table).  f32 rows on the spill table were measured and dropped:
// SIFT 1M at 10k queries 1.19 -> 1.47 ms, at 1k 0.55 -> 0.68 ms
// (profiles/r04/search_experiments/sift_spill_table_rejected.log).
template <int kSpace>
constexpr bool space_sq8() { return kSpace == 1 || kSpace == 2; }
template <int kSpace>
constexpr bool space_tab() { return kSpace == 2; }

template <int kChunks, int kSpace, int kMode = 0>
constexpr int search_min_waves() {
  if constexpr ((kMode & alaya_amd::kModeTwoWaves) != 0) return 2;  // the two-waves-per-SIMD wide-row kernels
  if constexpr (space_sq8<kSpace>()) {
    if (ALAYA_MIN_WAVES_SQ8 >= 0) return ALAYA_MIN_WAVES_SQ8;
    return kSpace == 2 && kChunks > 0 ? 4 : 0;
  }
  return kChunks > 0 && kChunks <= 8 ? ALAYA_MIN_WAVES_NARROW : (kChunks > 8 ? ALAYA_MIN_WAVES_WIDE : 0);
}

namespace alaya_amd {

namespace {

// LDS layout of a search workgroup of W waves: a shared region (SQ8: the per-index scale and min
// of SQ8Space's quantizer, identical for every query, stored once per workgroup) followed by one
// region of p.wave_lds bytes per wave (query, candidate batch, pool, visited table).
template <int kSpace>
__device__ __forceinline__ Lds carve_lds(const SearchParams &p, unsigned char *smem, int wave) {
  Lds L;
  unsigned char *ptr = smem + search_shared_lds_bytes(p.stride, space_sq8<kSpace>()) + static_cast<size_t>(wave) * p.wave_lds;
  L.q = reinterpret_cast<float *>(ptr);
  ptr += sq8_query_codes<kSpace>() ? (static_cast<size_t>(p.stride) + 15) / 16 * 16 : static_cast<size_t>(p.stride) * 4;
  L.cid = reinterpret_cast<uint32_t *>(ptr);
  ptr += 64 * 4;
  L.cd = reinterpret_cast<float *>(ptr);
  ptr += 64 * 4;
  L.sd = reinterpret_cast<float *>(ptr);
  ptr += 64 * 4;
  L.pd = reinterpret_cast<float *>(ptr);
  ptr += ((p.ef + 1) * 4 + 15) / 16 * 16;
  L.pi = reinterpret_cast<uint32_t *>(ptr);
  ptr += ((p.ef + 1) * 4 + 15) / 16 * 16;
  L.hash = reinterpret_cast<uint32_t *>(ptr);
  L.sq_scale = space_sq8<kSpace>() ? reinterpret_cast<float *>(smem) : nullptr;
  L.sq_min = space_sq8<kSpace>() ? reinterpret_cast<float *>(smem) + p.stride : nullptr;
  return L;
}

// SQ8: the workgroup's waves fill the shared scale / min once (SQ8Quantizer, sq8.hpp:99-130:
// scale = (max - min) * (1/255)), before any wave starts a query.
template <int kSpace>
__device__ __forceinline__ void fill_shared(const SearchParams &p, const Lds &L) {
  if constexpr (space_sq8<kSpace>()) {
    const float kInv255 = 1.0f / 255.0f;
    for (uint32_t e = threadIdx.x; e < p.stride; e += blockDim.x) {
      float sc = 0.f, mn = 0.f;
      if (e < p.dim) {
        mn = p.sq_min[e];
        sc = (p.sq_max[e] - mn) * kInv255;
      }
      L.sq_scale[e] = sc;
      L.sq_min[e] = mn;
    }
    __syncthreads();
  }
}

// Per-query setup shared by the search kernels: the query staged in LDS (SQ8: encoded with the
// quantizer), visited table and pool cleared, then Graph::initialize_search (graph.hpp:148-158).
// on_entry(has, id, d) sees what initialize_search hands to pool.insert, lane order = insertion order
// (the filtered search's result pool).
struct NoEntry {
  __device__ void operator()(bool, uint32_t, float) const {}
};

template <bool kIP, int kChunks, int kSpace, int kRows = 0, typename Entry = NoEntry>
__device__ __forceinline__ void query_begin(const SearchParams &p, const Lds &L, uint32_t qi, uint32_t *slot_bits,
                                            uint32_t *slot_dirty, uint16_t *slot_stab, Visited &vs, PoolState &ps,
                                            uint32_t &n_dist_up, uint32_t &n_hops_up, Entry on_entry = Entry()) {
  const int lane = lane_id();
  const uint32_t hsize = 1u << p.hash_log2;
  // ---- per-query init ------------------------------------------------------------------
  const float *qsrc = p.queries + static_cast<uint64_t>(qi) * p.q_stride;
  if constexpr (!space_sq8<kSpace>()) {
    for (uint32_t e = lane; e < p.stride; e += 64) L.q[e] = e < p.dim ? qsrc[e] : 0.f;
  } else {
    // SQ8Space::QueryComputer encodes the query with the quantizer (sq8_space.hpp:266-271,
    // SQ8Quantizer::quantize sq8.hpp:118-130), then every distance uses its codes.
    // (the per-index scale and min are the workgroup's shared LDS copy, fill_shared)
    for (uint32_t e = lane; e < p.stride; e += 64) {
      float xq = 0.f;
      uint32_t code = 0;
      if (e < p.dim) {
        const float v = qsrc[e];
        const float mn = p.sq_min[e];
        const float mx = p.sq_max[e];
        if (mx == mn) code = 0;
        else if (v >= mx) code = 255;
        else if (v <= mn) code = 0;
        else code = static_cast<uint8_t>(((v - mn) / (mx - mn)) * 255);
        const float xf = static_cast<float>(code);
        xq = kIP ? fmaf(xf, L.sq_scale[e], mn) : xf;
      }
      if constexpr (sq8_query_codes<kSpace>()) {
        reinterpret_cast<uint8_t *>(L.q)[e] = static_cast<uint8_t>(code);  // the term is rebuilt per chunk
      } else {
        L.q[e] = xq;
      }
    }
  }
  {
    const bool wide = p.vis_rbits == kVisWide;
    const uint32_t words = wide ? hsize : hsize / 2;
    for (uint32_t e = lane; e < words; e += 64) L.hash[e] = wide ? kEmpty : 0u;
  }
  for (uint32_t e = lane; e <= p.ef; e += 64) {
    L.pd[e] = 0.f;
    L.pi[e] = 0u;
  }
  wave_sync();
  vs = make_visited(p, L.hash, slot_bits, slot_dirty, slot_stab);
  ps = PoolState{0u, 0u, p.ef};
  constexpr bool kTab = space_tab<kSpace>();  // the kernels that may run on the spill table

  // ---- Graph::initialize_search (graph.hpp:148-158) ---------------------------------------
  if (p.levels != nullptr) {
    // OverlayGraph::initialize (overlay_graph.hpp:122-144): greedy descent, strict '<'.
    uint32_t u = p.ep;
    uint64_t off_u = p.upper_off[u];  // u's upper-level lists, kept while u stays
    if (lane == 0) L.cid[0] = u;
    wave_sync();
    space_distances<kIP, kChunks, kSpace, false, kRows>(p, L, L.cid, 1, L.cd);
    float cur = L.cd[0];
    ++n_dist_up;
    for (int level = static_cast<int>(p.levels[u]); level > 0; --level) {
      bool changed = true;
      while (changed) {
        changed = false;
        const uint32_t *list = p.upper_edges + off_u + static_cast<uint64_t>(level - 1) * p.upper_R;
        const uint32_t v = lane < static_cast<int>(p.upper_R) ? list[lane] : kEmpty;
        const uint64_t endm = ballot(lane < static_cast<int>(p.upper_R) && v == kEmpty);
        const int cnt = endm ? __ffsll(static_cast<unsigned long long>(endm)) - 1
                             : static_cast<int>(p.upper_R);
        ++n_hops_up;
        const bool has = lane < cnt;
        // every candidate's list offset is loaded beside its row: the hop to the winner then needs
        // one dependent load (its list), not two
        uint64_t off_v = 0;
        if (has) off_v = p.upper_off[v];
        wave_sync();
        if (has) L.cid[lane] = v;
        wave_sync();
        space_distances<kIP, kChunks, kSpace, false, kRows>(p, L, L.cid, cnt, L.cd);
        n_dist_up += cnt;
        // first index of the minimum == the sequential strict-'<' scan's final choice (the minimum
        // is order-free: DPP / swizzle steps within each 32-lane half, then the two halves)
        const float dl = has ? L.cd[lane] : FLT_MAX;
        float mn = dl;
        mn = fminf(mn, lane_xor<1>(mn));
        mn = fminf(mn, lane_xor<2>(mn));
        mn = fminf(mn, lane_xor<4>(mn));
        mn = fminf(mn, lane_xor<8>(mn));
        mn = fminf(mn, lane_xor<16>(mn));
        mn = fminf(read_lane(mn, 0), read_lane(mn, 32));
        const uint64_t at = ballot(has && dl == mn);
        if (at && mn < cur) {
          const int w = __ffsll(static_cast<unsigned long long>(at)) - 1;
          u = read_lane(v, w);
          off_u = (static_cast<uint64_t>(read_lane(static_cast<uint32_t>(off_v >> 32), w)) << 32) |
                  read_lane(static_cast<uint32_t>(off_v), w);
          cur = mn;
          changed = true;
        }
        wave_sync();
      }
    }
    // pool.insert(u, cur); vis.set(u)
    if (lane == 0) {
      L.pd[0] = cur;
      L.pi[0] = u;
    }
    ps.size = 1;
    ps.cur = 0;
    visit<kTab>(vs, u, lane == 0);
    wave_sync();
    on_entry(lane == 0, u, cur);
  } else {
    // NSG-style entry points: insert each ep, then mark it visited (graph.hpp:153-156)
    for (uint32_t b = 0; b < p.n_eps; b += 64) {
      const uint32_t cnt = min(64u, p.n_eps - b);
      const bool has = static_cast<uint32_t>(lane) < cnt;
      uint32_t v = has ? p.eps[b + lane] : 0u;
      if (has) L.cid[lane] = v;
      wave_sync();
      for (uint32_t c = 0; c < cnt; c += 8) {
        space_distances<kIP, kChunks, kSpace, false, kRows>(p, L, L.cid + c, min(8u, cnt - c), L.cd + c);
      }
      n_dist_up += cnt;
      const float d = has ? L.cd[lane] : 0.f;
      wave_sync();
      pool_merge(ps, L, has, v, d);
      on_entry(has, v, d);
      // duplicates among eps are all inserted (no visited check in the reference loop)
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t vj = read_lane(v, j);
        if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin<kTab>(vs);
        visit<kTab>(vs, vj, lane == 0);
      }
      wave_sync();
    }
  }
}

// Results (ids[i] = pool.id(i), distances[i] = pool.dist(i), graph_search_job.hpp:254-256) and the
// per-query counters.
__device__ __forceinline__ void query_end(const SearchParams &p, const Lds &L, const PoolState &ps, uint32_t qi,
                                          uint32_t n_dist, uint32_t n_expand, uint32_t n_dist_up,
                                          uint32_t n_hops_up) {
  const int lane = lane_id();
  for (uint32_t i = lane; i < p.k; i += 64) {
    uint32_t id = p.fill_id;
    float d = p.fill_id == kEmpty ? FLT_MAX : 0.f;  // kEmpty fill (shard / corrected rerank) sorts last
    if (i < ps.size) {
      id = L.pi[i] & kIdMask;
      d = L.pd[i];
    }
    p.out_ids[static_cast<uint64_t>(qi) * p.k + i] = id;
    if (p.out_dists) p.out_dists[static_cast<uint64_t>(qi) * p.k + i] = d;
  }
  if (p.out_counters && lane == 0) {
    uint32_t *c = p.out_counters + static_cast<uint64_t>(qi) * 4;
    c[0] = n_dist;
    c[1] = n_expand;
    c[2] = n_dist_up;
    c[3] = n_hops_up;
  }
}

// --------------------------------------------------------------------------------------------
// Distance helpers.  A searcher with no query left (the batch counter ran out) computes distances
// for the siblings of its workgroup that are still searching.  Each searcher keeps three requests on
// the workgroup's board: the node it is expanding (until it has read the memo) and the nodes it will
// most likely expand next -- the pool's first two unchecked entries right after each pop, and the
// merge's new next pop when it changes (the prediction holds ~99.8 % of the time for the next
// expansion).  Helpers claim 16 adjacency
// positions of a request at a time (older requests first: the nearer expansion), compute those
// rows' distances against the sibling's query and store (request seq, distance) per position in
// one memo, held in the region of the first wave that became a helper.  When the searcher expands
// a requested node it takes the memo's distance for every fresh neighbour whose entry carries the
// request's seq, and computes the rest itself -- none when the helpers kept up, so the expansion has
// no row gather at all.  The distances are deterministic (same function, same query vector, same
// row) and the searcher still does every visit, merge and pop itself, so ids, distances and
// counters are those of the search without helpers; a helper that falls behind or answers a stale
// request only costs work.  The reference keeps every worker busy to the end with its coroutine
// interleave (include/executor/worker.hpp:47,111-136); here the batch tail's idle waves (and, in
// batches smaller than the resident searchers, the spare ones) shorten the remaining searchers'
// expansions instead.
// LDS: a kHelpBoardBytes (256-byte) board after the workgroup's wave regions; the memo (W x kHelpSlots
// x R entries of 8 bytes) at byte p.memo_off of the memo wave's region -- its query vector or its pool
// and visited table, unused once it has no query.
// --------------------------------------------------------------------------------------------
// How far ahead a searcher asks: 1 = the next expansion, 2 = the next two (diagnostics builds:
// -DALAYA_HELP_DEPTH=2).  One slot more than the depth keeps the expanding node's request alive
// until its memo entries are read.
#ifndef ALAYA_HELP_DEPTH
#define ALAYA_HELP_DEPTH 1
#endif
// Issue priority (s_setprio) of a searcher with helpers present: a helper shares its SIMD with up to
// three waves of other workgroups, which may still be searching; the searchers' expansion chains run
// at this priority and helpers at 0, so a helper's distance work fills issue slots the chains leave
// free instead of delaying them.  0 = no priorities (diagnostics builds: -DALAYA_HELP_PRIO=0).
#ifndef ALAYA_HELP_PRIO
#define ALAYA_HELP_PRIO 2
#endif
constexpr int kHelpDepth = ALAYA_HELP_DEPTH;
static_assert(kHelpDepth == 1 || kHelpDepth == 2, "help depth 1 or 2");
constexpr int kHelpSlots = kHelpDepth + 1;  // requests per searcher
constexpr uint32_t kHelpClaim = 16;         // adjacency positions per claim (one row pass)
struct HelpOwner {                          // one searcher's requests
  uint64_t req[kHelpSlots];                 // (seq << 32) | node per slot; node kEmpty = none; seq only grows
  uint32_t claim[kHelpSlots];               // (seq mod 2^24) << 8 | next adjacency position to hand out
  uint32_t hits;                            // fresh distances taken from the memo (help_stats)
  uint32_t skips;                           // expansions whose fresh distances all came from the memo
  uint32_t rows;                            // as a helper: rows whose distances it computed
};
struct HelpBoard {
  HelpOwner own[4];
  uint32_t mask;  // bits 0-3: waves with no query left (helpers); bits 8-15: 1 + the memo wave
  uint32_t pad[3];
};
static_assert(sizeof(HelpBoard) <= kHelpBoardBytes, "board size");

__device__ __forceinline__ HelpBoard *help_board(const SearchParams &p, unsigned char *smem, int W) {
  return reinterpret_cast<HelpBoard *>(smem + search_shared_lds_bytes(p.stride, p.sq8_order != 0) +
                                       static_cast<size_t>(W) * p.wave_lds);
}

__device__ __forceinline__ void help_board_init(HelpBoard *b) {
  for (int i = 0; i < 4; ++i) {
    for (int s = 0; s < kHelpSlots; ++s) {
      b->own[i].req[s] = static_cast<uint64_t>(kEmpty);
      b->own[i].claim[s] = 0u;
    }
    b->own[i].hits = 0u;
    b->own[i].skips = 0u;
    b->own[i].rows = 0u;
  }
  b->mask = 0u;
}

__device__ __forceinline__ uint32_t help_word(HelpBoard *b) {
  return read_lane(__hip_atomic_load(&b->mask, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP), 0);
}

// A searcher's requests as (node, seq) pairs (wave-uniform; each pair is one 8-byte LDS word)
struct HelpReqs {
  uint32_t node[kHelpSlots];
  uint32_t seq[kHelpSlots];
};
__device__ __forceinline__ HelpReqs help_reqs(HelpBoard *b, int t) {
  HelpReqs q;
#pragma unroll
  for (int s = 0; s < kHelpSlots; ++s) {
    const uint64_t r = __hip_atomic_load(&b->own[t].req[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    q.node[s] = read_lane(static_cast<uint32_t>(r), 0);
    q.seq[s] = read_lane(static_cast<uint32_t>(r >> 32), 0);
  }
  return q;
}

// A new query: no request of the previous one may match again (memo entries are tagged with a seq
// that only grows; emptied slots are skipped by the helpers).
__device__ __forceinline__ void help_reset(HelpBoard *b, int wave) {
  if (lane_id() < kHelpSlots)
    __hip_atomic_store(&b->own[wave].req[lane_id()], static_cast<uint64_t>(kEmpty), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The searcher has read the memo for slot s: no helper should start more work on that request.
__device__ __forceinline__ void help_retire(HelpBoard *b, int wave, int s, uint32_t seq) {
  if (lane_id() == 0)
    __hip_atomic_store(&b->own[wave].claim[s], ((seq & 0xffffffu) << 8) | 0xffu, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The searcher's side of the board, kept in (scalar) registers so that an expansion pays no LDS
// round trip for it: its requests, its seq counter and the memo wave (-1 while it has no helper).
struct HelpMine {
  uint32_t node[kHelpSlots];
  uint32_t seq[kHelpSlots];
  uint32_t next_seq;
  int memo_wave;
};

// A new request for `node` in slot s (lane 0: the claim word first, then the request, so a helper
// that sees the request finds its claim reset).
__device__ __forceinline__ void mine_publish(HelpBoard *b, int wave, HelpMine &m, int s, uint32_t node) {
  const uint32_t seq = ++m.next_seq;
  m.node[s] = node;
  m.seq[s] = seq;
  if (lane_id() == 0) {
    HelpOwner &o = b->own[wave];
    // the LDS performs one wave's operations in order: a compiler barrier keeps the claim before the
    // request without the release's wait for every outstanding LDS and scalar load
    __hip_atomic_store(&o.claim[s], (seq & 0xffffffu) << 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
    __hip_atomic_store(&o.req[s], (static_cast<uint64_t>(seq) << 32) | node, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// Requests for the next expansions c1 (and, at depth 2, c2; kEmpty: none), keeping the slot of the
// node being expanded (u) until its memo entries are read: slots holding u, c1 or c2 stay, the others
// take the missing ones (with depth + 1 slots there is always room).
__device__ __forceinline__ void mine_request(HelpBoard *b, int wave, HelpMine &m, uint32_t u, uint32_t c1,
                                             uint32_t c2) {
  if (kHelpDepth < 2) c2 = kEmpty;
  bool need1 = c1 != kEmpty, need2 = c2 != kEmpty && c2 != c1;
#pragma unroll
  for (int s = 0; s < kHelpSlots; ++s) {
    need1 = need1 && m.node[s] != c1;
    need2 = need2 && m.node[s] != c2;
  }
  if (!need1 && !need2) return;
#pragma unroll
  for (int s = 0; s < kHelpSlots; ++s) {
    const uint32_t x = m.node[s];
    if (x != kEmpty && (x == u || x == c1 || x == c2)) continue;  // a slot to keep
    if (need1) {
      mine_publish(b, wave, m, s, c1);
      need1 = false;
    } else if (need2) {
      mine_publish(b, wave, m, s, c2);
      need2 = false;
    }
  }
}

__device__ __forceinline__ void mine_reset(HelpBoard *b, int wave, HelpMine &m) {
#pragma unroll
  for (int s = 0; s < kHelpSlots; ++s) m.node[s] = kEmpty;
  help_reset(b, wave);
}

// The memo: W x kHelpSlots x R entries (seq << 32 | distance bits) at p.memo_off of the memo wave's
// region.
template <int kSpace>
__device__ __forceinline__ uint64_t *help_memo(const SearchParams &p, unsigned char *smem, int memo_wave) {
  return reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(carve_lds<kSpace>(p, smem, memo_wave).q) +
                                      p.memo_off);
}

// n_got of an expansion's nf fresh distances came from the memo.
__device__ __forceinline__ void help_count(HelpBoard *b, int wave, uint32_t n_got, uint32_t nf, int lane) {
  if (lane == 0 && n_got) {
    b->own[wave].hits += n_got;
    if (n_got == nf) b->own[wave].skips += 1u;
  }
}

// A searcher's help_stats row (the board outlives every wave's searching).
__device__ __forceinline__ void help_stats_out(const SearchParams &p, const HelpBoard *b, int wave, uint64_t slot, int lane) {
  if (p.help_stats != nullptr && lane == 0) {
    p.help_stats[3 * slot] = b->own[wave].hits;
    p.help_stats[3 * slot + 1] = b->own[wave].skips;
    p.help_stats[3 * slot + 2] = b->own[wave].rows;
  }
}

// Whether sibling t has probably visited v already (a hint: read while the sibling writes, so it may
// be stale either way): its LDS first level, and -- SQ8 on the spill table -- its spill-table bucket.
template <int kSpace>
__device__ __forceinline__ bool sibling_visited(const SearchParams &p, const Lds &Lt, int t, uint32_t v, bool want) {
  Visited vt = make_visited(p, Lt.hash, nullptr, nullptr, nullptr);
  bool seen = want && table_lookup<true>(vt, v);
  if constexpr (space_tab<kSpace>()) {
    if (p.spill_table != nullptr) {
      const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + t;
      vt.stab = p.spill_table + (slot << p.stab_log2);
      vt.stab_bmask = (1u << (p.stab_log2 - 3)) - 1u;
      uint32_t home, code;
      stab_key(vt, v, home, code);
      uint64_t lo = 0ull, hi = 0ull;
      if (want && !seen) stab_load(vt, home, lo, hi);
      bool found;
      uint32_t occ;
      stab_scan(lo, hi, code, found, occ);
      seen = seen || (want && found);
    }
  }
  return seen;
}

// A wave whose batch counter ran out helps its siblings until every wave of the workgroup has none
// left (then all exit: no wave ever waits for another).
template <bool kIP, int kChunks, int kSpace>
__device__ void help_siblings(const SearchParams &p, unsigned char *smem, const Lds &L, HelpBoard *b, int wave,
                              int W) {
  const int lane = lane_id();
  const uint32_t R = p.R;
  const uint32_t full = (1u << W) - 1u;
  if constexpr (ALAYA_HELP_PRIO > 0) __builtin_amdgcn_s_setprio(0);  // helpers yield to searchers
  // the visited hint (skip rows the sibling has already visited): by default where a stale read costs
  // a global round trip less than the rows it saves -- SQ8 on the spill table (config 5, 1k queries:
  // 3.47 ms with it, 3.62 without); the f32 rows of the SIFT shape are cheaper to compute than to
  // filter (10k queries: 1.138 ms without, 1.153 with).  ALAYA_HELP_FLAGS bit 0 / 1 force it off / on.
  const bool hint = (p.help_flags & 2u) || (space_sq8<kSpace>() && !(p.help_flags & 1u));
  uint32_t *exhausted = reinterpret_cast<uint32_t *>(L.sd);  // per (sibling, slot): a request fully claimed
  if (lane < 4 * kHelpSlots) exhausted[lane] = 0u;
  // Leave the searchers first: retire this wave's last requests and set its helper bit, so no helper
  // that reads the board from now on picks this wave as a sibling.  Only then may its region be
  // overwritten by the memo clear below (with memo_off > 0 it covers the pool and the visited
  // table, which another helper's visited hint reads; a helper that read the board just before
  // still probes a bounded lap, table_lookup<true>).
  help_reset(b, wave);
  wave_sync();
  if (lane == 0) __hip_atomic_fetch_or(&b->mask, 1u << wave, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  wave_sync();
  // the first helper's region holds the memo: clear this wave's (seq 0 = no entry), then claim the
  // role (no helper reads the memo before some wave has claimed it: each claims or finds it claimed
  // before its own loop, and a searcher looks only once the role is set)
  {
    uint64_t *mine = help_memo<kSpace>(p, smem, wave);
    for (uint32_t e = lane; e < static_cast<uint32_t>(W) * kHelpSlots * R; e += 64)
      __hip_atomic_store(mine + e, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  wave_sync();
  if (lane == 0) {
    uint32_t cur = __hip_atomic_load(&b->mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while ((cur >> 8) == 0u) {
      const uint32_t want = cur | (static_cast<uint32_t>(wave + 1) << 8);
      if (__hip_atomic_compare_exchange_strong(&b->mask, &cur, want, __ATOMIC_RELEASE, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP))
        break;
    }
  }
  wave_sync();
  int t = wave;
  for (;;) {
    const uint32_t hw = help_word(b);
    const uint32_t mask = hw & 0xffu;
    if (mask == full) break;  // every sibling is done
    uint64_t *memo = help_memo<kSpace>(p, smem, static_cast<int>(hw >> 8) - 1);
    do {
      t = t + 1 == W ? 0 : t + 1;
    } while ((mask >> t) & 1u);
    const HelpReqs r = help_reqs(b, t);
    // the oldest open request first (the nearest expansion)
    uint32_t order = 0u;  // slot indices, 2 bits each, oldest first
    if constexpr (kHelpSlots == 2) {
      order = r.seq[1] < r.seq[0] ? (1u | (0u << 2)) : (0u | (1u << 2));
    } else {
      const uint32_t a = r.seq[0], b1 = r.seq[1], c = r.seq[kHelpSlots - 1];
      const int s0 = (a <= b1 && a <= c) ? 0 : (b1 <= c ? 1 : 2);
      const int sa = (s0 + 1) % 3, sb = (s0 + 2) % 3;
      const bool swap = r.seq[sb] < r.seq[sa];
      order = static_cast<uint32_t>(s0) | (static_cast<uint32_t>(swap ? sb : sa) << 2) |
              (static_cast<uint32_t>(swap ? sa : sb) << 4);
    }
    bool worked = false;
    for (int k = 0; k < kHelpSlots && !worked; ++k) {
      const int s = static_cast<int>((order >> (2 * k)) & 3u);
      const uint32_t node = r.node[s], seq = r.seq[s];
      if (node == kEmpty || seq == 0u || exhausted[t * kHelpSlots + s] == seq) continue;
      uint32_t old = 0u;
      if (lane == 0) old = atomicAdd(&b->own[t].claim[s], kHelpClaim);
      old = read_lane(old, 0);
      if ((old >> 8) != (seq & 0xffffffu)) continue;  // replaced by a newer request meanwhile
      const uint32_t pos = old & 0xffu;
      const uint32_t v = adjacency_row(p, static_cast<int>(R), node);
      const uint32_t cnt = static_cast<uint32_t>(adjacency_count(static_cast<int>(R), v));
      if (pos >= cnt) {
        if (lane == 0) exhausted[t * kHelpSlots + s] = seq;
        wave_sync();
        continue;
      }
      worked = true;
      const Lds Lt = carve_lds<kSpace>(p, smem, t);
      bool want = static_cast<uint32_t>(lane) >= pos && static_cast<uint32_t>(lane) < min(pos + kHelpClaim, cnt);
      if (hint) want = want && !sibling_visited<kSpace>(p, Lt, t, v, want);
      const uint64_t wm = ballot(want);
      const int n = __popcll(wm);
      if (n == 0) continue;
      const uint32_t slot = __popcll(wm & ((1ull << lane) - 1ull));
      if (want) L.cid[slot] = v;
      wave_sync();
      space_distances<kIP, kChunks, kSpace>(p, Lt, L.cid, n, L.cd);
      if (lane == 0) b->own[wave].rows += static_cast<uint32_t>(n);
      if (want) {
        const uint64_t e = (static_cast<uint64_t>(seq) << 32) | __float_as_uint(L.cd[slot]);
        __hip_atomic_store(memo + (static_cast<uint32_t>(t) * kHelpSlots + s) * R + lane, e, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      wave_sync();
    }
    if (!worked) __builtin_amdgcn_s_sleep(4);  // ~256 cycles: polls stay off the searchers' LDS
  }
}

// --------------------------------------------------------------------------------------------
// Scout (SearchParams::scout; the two-waves screening kernels under the integer screen).  A workgroup is
// Ws searcher waves followed by Ws scout waves; scout wave Ws + i serves searcher i and owns nothing
// but registers.  The searcher posts the nodes it will probably pop next -- the pool's first two
// unchecked entries after each pop, and the merge's new next pop when that changes -- as requests on
// its board.  The scout loads a requested node's adjacency row, drops the neighbours the searcher's
// first-level visited table already holds (a hint: a stale answer costs bytes or a miss), runs one pass
// of the integer screen over the others' records with its own copy of the query's codes, and writes one
// bound per adjacency position into the request's memo row.  When the searcher pops a node whose row
// is published it takes its fresh candidates' bounds from there and skips the screen pass.
//
// Why the bound is the same: screen_int_bound is a function of the query (its codes, sums, grid and
// error, which screen_query_codes derives from L.q alone) and of one row's record, which no launch
// writes.  It depends on neither tau, the pool nor the visited set, so the value computed early by
// another wave has the bits the searcher would compute at the pop; everything after it -- keep, the
// counters, the exact pass, the merge -- runs in the searcher as before.
//
// Protocol (all workgroup-scope relaxed atomics; the LDS performs one wave's operations in order, so
// compiler barriers are the only fences).  The searcher keeps none of it in registers: its kernel has
// none to spare at two waves per SIMD.
//   * state: 0 between queries, the query's epoch (its index + 1) while L.q holds that query,
//     kScoutDone once the searcher has no query left.  The searcher zeroes it before it overwrites L.q
//     and sets the new epoch after, so a scout that reads the same epoch before and after reading L.q
//     (or the requests) read them within that query.
//   * req[0 .. 2] = the node being expanded (kEmpty once its memo row has been looked at), the next pop
//     and the one after (kEmpty: none).  The scout answers the next pop first, and writes only into a
//     row that answers none of the three.
//   * tag[s] = epoch << 32 | node of the request row s answers, 0 while it is being written: the scout
//     zeroes the tag, writes the bounds, then sets the tag; the searcher finds its row by the tag, reads
//     its bounds and the tag again, and takes the bounds only if both reads show its (query, node).  A
//     bound depends on nothing else, so a row answers its node for as long as the query lasts, and the
//     epoch keeps one query's rows from the next.
// No wave waits for another's data: a searcher never waits at all, and a scout leaves its poll loop
// when it reads kScoutDone, which its searcher -- a wave of the same workgroup, so co-resident --
// stores on its only way out of the query loop.
// --------------------------------------------------------------------------------------------
constexpr uint32_t kScoutDone = 0xffffffffu;
constexpr uint32_t kScoutMissing = 0xffffffffu;  // a memo bound the scout did not compute (never a bound's bits: a NaN)
constexpr uint64_t kScoutNoMatch = 1ull << 63;   // kScoutMiss: set in every tag the scout writes; no lookup has it
struct ScoutBoard {
  uint64_t tag[kScoutSlots];
  uint32_t bound[kScoutSlots][kScoutR];
  uint32_t req[kScoutSlots];
  uint32_t state;
  uint32_t stat[3];  // the searcher's counters: expansions that screened, memo hits, verify mismatches
  uint32_t early;    // kScoutEarly's two (each stops at 0xffff): low half early requests, high half confirmed
};
static_assert(sizeof(ScoutBoard) == kScoutBoardBytes && kScoutSlots == 3, "board size");

__device__ __forceinline__ ScoutBoard *scout_board(const SearchParams &p, unsigned char *smem, int n_search, int i) {
  return reinterpret_cast<ScoutBoard *>(smem + search_shared_lds_bytes(p.stride, p.sq8_order != 0) +
                                        static_cast<size_t>(n_search) * p.wave_lds) + i;
}

template <typename T>
__device__ __forceinline__ T lds_load(const T *a) {
  return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <typename T, typename U>
__device__ __forceinline__ void lds_store(T *a, U v) {
  __hip_atomic_store(a, static_cast<T>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// keeps the compiler from moving LDS accesses across it; the LDS itself keeps a wave's order
__device__ __forceinline__ void lds_order() { asm volatile("" ::: "memory"); }

__device__ __forceinline__ uint64_t scout_key(uint32_t epoch, uint32_t node) {
  return (static_cast<uint64_t>(epoch & 0x7fffffffu) << 32) | node;
}

// The searcher's requests: lanes 0 .. 2 store (a, b, c) into req[first ..]; kEmpty = none.
__device__ __forceinline__ void scout_post(ScoutBoard *b, int first, int n, uint32_t x0, uint32_t x1, uint32_t x2) {
  const int lane = lane_id();
  if (lane < n) lds_store(&b->req[first + lane], lane == 0 ? x0 : (lane == 1 ? x1 : x2));
}

// ---- the searcher's side of the protocol ----
// Before the roles part (a workgroup barrier follows): the searcher's first lanes clear its board.
__device__ __forceinline__ void scout_board_init(ScoutBoard *b) {
  const int lane = lane_id();
  if (lane < static_cast<int>(kScoutSlots)) {
    b->req[lane] = kEmpty;
    b->tag[lane] = 0ull;
    b->stat[lane] = 0u;
    b->state = 0u;
    b->early = 0u;
  }
}

// Between queries: L.q is about to change, and no request of the last query stays.
__device__ __forceinline__ void scout_query_end(ScoutBoard *b) {
  if (lane_id() == 0) lds_store(&b->state, 0u);
  lds_order();
  scout_post(b, 0, 3, kEmpty, kEmpty, kEmpty);
}

// L.q holds the query of this epoch until the next scout_query_end.
__device__ __forceinline__ void scout_query_begin(ScoutBoard *b, uint32_t epoch) {
  lds_order();
  if (lane_id() == 0) lds_store(&b->state, epoch);
}

// The bounds of node u's neighbours, if a memo row is published for it -- tag, bounds, tag again; a
// fresh lane reads its own adjacency position and hands the bound to the lane that will hold the
// candidate (cd[slot]).  One bound missing: false, and the searcher's own pass for the whole list.
__device__ __forceinline__ bool scout_lookup(ScoutBoard *b, uint32_t epoch, uint32_t u, bool fresh, uint32_t slot, float *cd) {
  const int lane = lane_id();
  bool memo_ok = false;
  const uint64_t key = scout_key(epoch, u);
  uint64_t tg = 0ull;
  if (lane < static_cast<int>(kScoutSlots)) tg = lds_load(&b->tag[lane]);
  const uint64_t rows = ballot(tg == key);
  if (rows != 0ull) {
    const int row = __ffsll(static_cast<unsigned long long>(rows)) - 1;
    lds_order();
    const uint32_t mb = lds_load(&b->bound[row][lane & static_cast<int>(kScoutR - 1)]);
    lds_order();
    const uint64_t again = lds_load(&b->tag[row]);
    memo_ok = ballot(again != key || (fresh && (mb == kScoutMissing || lane >= static_cast<int>(kScoutR)))) == 0ull;
    if (memo_ok && fresh) cd[slot] = __uint_as_float(mb);
  }
  if (lane == 0) lds_store(&b->req[0], kEmpty);  // looked at: the scout may reuse u's row
  return memo_ok;
}

// An expansion that screened, from the memo (hit) or with the searcher's own pass.
__device__ __forceinline__ void scout_count_screen(ScoutBoard *b, bool hit) {
  if (lane_id() == 0) {
    b->stat[0] += 1u;
    if (hit) b->stat[1] += 1u;
  }
}

// kScoutEarly: a survivor whose distance comes out below the first unchecked entry's is the next pop,
// and the merge names it only after the exact pass and most of its own work.  The survivor with the
// smallest bound (none = 0 = smallest) is the likely one: if its bound is below that entry's distance
// it is requested now, the entry itself (pred) as the pop after.  A hint like every request: a wrong
// one costs the scout a row, and scout_retarget still posts what the merge finds.
__device__ __forceinline__ void scout_early_request(ScoutBoard *b, const Lds &L, const PoolState &ps, bool keep, float lb3,
                                                    uint32_t c, uint32_t pred) {
  const uint32_t kb = keep ? (lb3 > 0.f ? __float_as_uint(lb3) : 0u) : 0xffffffffu;
  uint32_t mn = min(kb, lane_xor<1>(kb));
  mn = min(mn, lane_xor<2>(mn));
  mn = min(mn, lane_xor<4>(mn));
  mn = min(mn, lane_xor<8>(mn));
  mn = min(mn, lane_xor<16>(mn));
  mn = min(read_lane(mn, 0), read_lane(mn, 32));
  if (__uint_as_float(mn) < L.pd[ps.cur]) {
    const uint32_t cand = read_lane(c, __ffsll(static_cast<unsigned long long>(ballot(kb == mn))) - 1);
    scout_post(b, 1, 2, cand, pred, kEmpty);
    if (lane_id() == 0 && (b->early & 0xffffu) != 0xffffu) b->early += 1u;
  }
}

// kScoutVerify: bounds of the searcher's own that did not have the bits of the memo's.
__device__ __forceinline__ void scout_count_mismatches(ScoutBoard *b, uint32_t bad, int lane) {
  if (lane == 0 && bad != 0u) b->stat[2] += bad;
}

// The merge found the next pop nx: requested, with the old prediction as the pop after.
__device__ __forceinline__ void scout_retarget(ScoutBoard *b, bool early, uint32_t nx, uint32_t old_pred) {
  // (an early request that named nx: req[1] holds nx only then, the pop's own post was pred)
  if (early && lane_id() == 0 && lds_load(&b->req[1]) == nx && (b->early >> 16) != 0xffffu) b->early += 0x10000u;
  scout_post(b, 1, 2, nx, old_pred, kEmpty);
}

// The searcher's only way out of the query loop: the scout leaves its poll loop.  The scout itself
// writes word 2 of both stats rows (the records it read, the nodes it dropped).
__device__ __forceinline__ void scout_leave(const SearchParams &p, ScoutBoard *b, uint64_t slot) {
  const int lane = lane_id();
  if (lane == 0) lds_store(&b->state, kScoutDone);
  if (p.scout_stats != nullptr && lane == 0) {
    p.scout_stats[4 * slot] = b->stat[0];
    p.scout_stats[4 * slot + 1] = b->stat[1];
    p.scout_stats[4 * slot + 3] = b->stat[2];
  }
  if (p.scout_policy_stats != nullptr && lane == 0) {
    p.scout_policy_stats[3 * slot] = b->early & 0xffffu;
    p.scout_policy_stats[3 * slot + 1] = b->early >> 16;
  }
}

// The scout wave of the searcher whose LDS region is Ls.
template <int kChunks>
__device__ void scout_loop(const SearchParams &p, const Lds &Ls, ScoutBoard *b, uint64_t slot) {
  uint32_t *stats = p.scout_stats != nullptr ? p.scout_stats + 4 * slot : nullptr;
  uint32_t *policy_stats = p.scout_policy_stats != nullptr ? p.scout_policy_stats + 3 * slot : nullptr;
  const int lane = lane_id();
  const int mine = screen_pass_row(lane);           // the adjacency position lane (& 31) finishes
  const int R = static_cast<int>(p.R);              // <= kScoutR (the plan)
  const uint32_t rec = screen_u8_record_bytes(p.stride);
  const bool miss = (p.scout & kScoutMiss) != 0u;
  const bool recheck = (p.scout_policy & kScoutRecheck) != 0u;
  __builtin_amdgcn_s_setprio(0);                     // the scout fills issue slots the searchers leave free
  ScreenQuery sq{};
  uint32_t sq_epoch = 0u;
  uint32_t records = 0u, abandoned = 0u;
  for (;;) {
    const uint32_t e = read_lane(lds_load(&b->state), 0);
    if (e == kScoutDone) break;
    if (e == 0u) {
      __builtin_amdgcn_s_sleep(8);
      continue;
    }
    if (e != sq_epoch) {  // a new query: its codes, valid only if L.q held it all the while
      lds_order();
      sq = screen_query_codes<kChunks>(p, Ls.q);
      lds_order();
      sq_epoch = read_lane(lds_load(&b->state), 0) == e ? e : 0u;
      continue;
    }
    uint32_t rq = kEmpty;
    uint64_t tg = 0ull;
    if (lane < static_cast<int>(kScoutSlots)) {
      rq = lds_load(&b->req[lane]);
      tg = lds_load(&b->tag[lane]);
    }
    lds_order();
    if (read_lane(lds_load(&b->state), 0) != sq_epoch) continue;  // the requests may be another query's
    const uint32_t u = read_lane(rq, 0), c1 = read_lane(rq, 1), c2 = read_lane(rq, 2);
    // the rows as (query, node), whatever kScoutMiss marked them with
    const uint64_t ku = scout_key(e, u), k1 = scout_key(e, c1), k2 = scout_key(e, c2);
    tg &= ~kScoutNoMatch;
    const bool have1 = ballot(tg == k1) != 0ull, have2 = ballot(tg == k2) != 0ull;
    // the next pop before the one after (kScoutMiss: only ever the one after)
    uint32_t node = kEmpty;
    if (!miss && c1 != kEmpty && !have1) {
      node = c1;
    } else if (c2 != kEmpty && !have2) {
      node = c2;
    }
    // a row that answers none of the three requests; none: the searcher has yet to look at u's
    const uint64_t spare = ballot(lane < static_cast<int>(kScoutSlots) && tg != ku && tg != k1 && tg != k2);
    if (node == kEmpty || spare == 0ull) {
      __builtin_amdgcn_s_sleep(8);  // ~512 cycles: polls stay off the searcher's LDS
      continue;
    }
    const int row = __ffsll(static_cast<unsigned long long>(spare)) - 1;
    // lanes 0 .. 31 take one adjacency position each, the one whose sum the pass leaves them
    const uint32_t v = adjacency_row(p, R, node);
    const int cnt = adjacency_count(R, v);
    bool want = lane < cnt;
    want = want && !sibling_visited<0>(p, Ls, 0, v, want);
    const uint64_t wm = ballot(want);
    // kScoutRecheck: the adjacency row took a round trip, and the searcher may have merged, popped or
    // retargeted meanwhile.  A node that is no longer the next pop or the one after costs its 128 B
    // adjacency row and no record; the loop goes on with the requests as they stand now.
    if (recheck) {
      lds_order();
      uint32_t rq2 = kEmpty;
      if (lane < static_cast<int>(kScoutSlots)) rq2 = lds_load(&b->req[lane]);
      lds_order();
      const uint32_t e2 = read_lane(lds_load(&b->state), 0);
      if (e2 != e || (read_lane(rq2, 1) != node && read_lane(rq2, 2) != node)) {
        ++abandoned;
        continue;
      }
    }
    if (lane == 0) lds_store(&b->tag[row], 0ull);
    lds_order();
    uint32_t lb_bits = kScoutMissing;
    if (wm != 0ull) {
      const uint32_t v0 = read_lane(v, __ffsll(static_cast<unsigned long long>(wm)) - 1);
      const uint32_t id = want ? v : v0;  // an unwanted slot repeats the first wanted row
      const uint32_t idm = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(mine << 2, static_cast<int>(id)));
      const uint8_t *rp = p.screen_u8 + static_cast<uint64_t>(idm) * rec;
      const float4 head = *reinterpret_cast<const float4 *>(rp);
      const uint2 sums = *reinterpret_cast<const uint2 *>(rp + screen_u8_sums_offset(p.stride));
      const uint32_t ac = screen_dots_pass<kChunks>(p, sq.codes, id, NoHook());
      const float lb = screen_int_bound(p.stride, sq.err, sq.lo, sq.scale, sq.a1, sq.a2, head.x, head.y, head.z, sums.x,
                                        sums.y, ac);
      if ((wm >> mine) & 1ull) lb_bits = __float_as_uint(lb);
      records += static_cast<uint32_t>(__popcll(wm));
    }
    if (lane < 32 && mine < R) lds_store(&b->bound[row][mine], lb_bits);
    lds_order();
    if (lane == 0) lds_store(&b->tag[row], scout_key(e, node) | (miss ? kScoutNoMatch : 0ull));
  }
  if (stats != nullptr && lane == 0) stats[2] = records;
  if (policy_stats != nullptr && lane == 0) policy_stats[2] = abandoned;
}

// A searcher's screen_stats row: every searcher of the launch writes its slot.
__device__ __forceinline__ void screen_stats_out(const SearchParams &p, uint64_t slot, uint32_t n_screened,
                                                 uint32_t n_screened_out, int lane) {
  if (p.screen_stats != nullptr && lane == 0) {
    p.screen_stats[2 * slot] = n_screened;
    p.screen_stats[2 * slot + 1] = n_screened_out;
  }
}

// --------------------------------------------------------------------------------------------
// The search kernel.
// --------------------------------------------------------------------------------------------
// kMode is a set of the kMode* bits of search_variants.h, which also lists the instantiations.
// A workgroup holds blockDim.x / 64 waves (1 for wide f32 rows; 4 for SQ8, which share the
// quantizer's scale / min, and for searches with helpers); each wave is an independent persistent
// searcher with its own visited spill slot.  After fill_shared the waves never wait on each other.
template <bool kIP, int kChunks, int kMode, int kSpace = 0>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(search_min_waves<kChunks, kSpace, kMode>() ? search_min_waves<kChunks, kSpace, kMode>() : 1,
                                       8))) hnsw_search_kernel(SearchParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool kStamp = (kMode & kModeStamp) != 0;
  constexpr bool kCheck = (kMode & kModeCheck) != 0;
  constexpr bool kHelp = (kMode & kModeHelp) != 0;
  constexpr int kRows = (kMode & kModeTwoWaves) != 0 ? 1 : 0;
  // Candidate screen (f32 L2 rows of d >= 512, no helpers): rows per lane group of the f16 pass --
  // 4 (32 candidates, a whole expansion of an R = 32 graph, in 2 kChunks float4 of registers), or 2
  // in the two-waves-per-SIMD kernels' half register budget.
  constexpr bool kScreen = (kMode & kModeScreen) != 0;
  static_assert(!kScreen || (kSpace == 0 && !kIP && !kHelp && kChunks >= 16 && kChunks % 2 == 0), "screen: wide f32 L2 rows");
  constexpr int kScreenRows = (kMode & kModeTwoWaves) != 0 ? 2 : 4;
  // the 8-bit records (p.screen == 2) hold a row in half the registers: 4 rows in both kernels
  constexpr int kScreenRowsU8 = 4;
  uint32_t n_screened = 0, n_screened_out = 0;  // wave-uniform, over the searcher's queries
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x >> 6);
  // Scout (p.scout, wave-uniform, the two-waves screening kernels only): the workgroup's upper half are
  // scout waves, one per searcher wave.  The roles part here, before any per-query state exists; no
  // workgroup barrier runs after it.
  constexpr bool kScout = kScreen && (kMode & kModeTwoWaves) != 0;
  const bool scouting = kScout && p.scout != 0u;
  const bool early = scouting && p.screen == 3 && (p.scout_policy & kScoutEarly) != 0u;
  const int W = static_cast<int>(blockDim.x >> 6) >> (scouting ? 1 : 0);  // searcher waves
  ScoutBoard *sboard = nullptr;
  if constexpr (kScout) {
    if (scouting) {
      sboard = scout_board(p, smem, W, wave < W ? wave : wave - W);
      if (wave < W) scout_board_init(sboard);
      __syncthreads();
      if (wave >= W) {
        scout_loop<kChunks>(p, carve_lds<kSpace>(p, smem, wave - W), sboard,
                            static_cast<uint64_t>(blockIdx.x) * W + (wave - W));
        return;
      }
      __builtin_amdgcn_s_setprio(2);  // the searcher's chain issues ahead of the scout that shares its SIMD
    }
  }
  const Lds L = carve_lds<kSpace>(p, smem, wave);
  fill_shared<kSpace>(p, L);
  HelpBoard *board = kHelp ? help_board(p, smem, W) : nullptr;
  HelpMine mine;
  if constexpr (kHelp) {
    if constexpr (ALAYA_HELP_PRIO > 0) __builtin_amdgcn_s_setprio(ALAYA_HELP_PRIO);
    if (threadIdx.x == 0) help_board_init(board);
    __syncthreads();
    for (int s = 0; s < kHelpSlots; ++s) mine.node[s] = kEmpty, mine.seq[s] = 0u;
    mine.next_seq = 0u;
    mine.memo_wave = -1;
  }
  const uint64_t bit_words = (p.n + 31) / 32;
  const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * W + wave;
  uint32_t *slot_bits = p.overflow_bits + slot * bit_words;
  uint32_t *slot_dirty = p.dirty_words + slot * p.dirty_cap;
  // spill tables only in the AVX-512-order SQ8 kernels (a compile-time null elsewhere: the f32
  // kernels carry none of it)
  uint16_t *slot_stab = (space_tab<kSpace>() && p.spill_table) ? p.spill_table + (slot << p.stab_log2) : nullptr;

  bool first_round = true;
  for (;;) {
    uint32_t qi = 0;
    if (kHelp && first_round) {
      // first round assigned wave-major over the workgroups, so a batch smaller than the resident
      // searchers leaves every workgroup a mix of searchers and helpers; then the work counter
      qi = static_cast<uint32_t>(wave) * gridDim.x + blockIdx.x;
    } else {
      if (lane == 0) qi = atomicAdd(p.work_counter, 1u);
      qi = read_lane(qi, 0) + (kHelp ? static_cast<uint32_t>(W) * gridDim.x : 0u);
    }
    first_round = false;
    if (qi >= p.nq) break;
    // a memo entry belongs to the query it was requested in: requests of an earlier query never
    // match again (the seq only grows, and the requests are dropped here)
    if constexpr (kHelp) mine_reset(board, wave, mine);
    if constexpr (kScout) {
      if (scouting) scout_query_end(sboard);
    }

    uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t_prev = kStamp ? __builtin_readcyclecounter() : 0;
    const uint64_t t_begin = t_prev;
    auto stamp = [&](int slot) {
      if constexpr (kStamp) {
        const uint64_t now = __builtin_readcyclecounter();
        st[slot] += now - t_prev;
        t_prev = now;
      }
    };
    Visited vs;
    PoolState ps;
    uint32_t n_dist = 0, n_expand = 0, n_dist_up = 0, n_hops_up = 0;
    query_begin<kIP, kChunks, kSpace, kRows>(p, L, qi, slot_bits, slot_dirty, slot_stab, vs, ps, n_dist_up, n_hops_up);
    ScreenQuery sq{};  // the integer screen's view of the query (p.screen == 3), in registers
    if constexpr (kScreen) {
      if (p.screen == 3) sq = screen_query_codes<kChunks>(p, L.q);
    }
    if constexpr (kScout) {
      if (scouting) scout_query_begin(sboard, qi + 1u);
    }

    // ---- best-first expansion (graph_search_job.hpp:228-252 / 310-330) -----------------------
    stamp(0);
    // Adjacency prefetch (no semantic effect): after a pop, the first unchecked entry is the next
    // expansion unless the merge puts a closer candidate in front of it.  Its 128 B row is loaded
    // into registers while this expansion runs and used only if the next pop returns that id.
    uint32_t pred = kEmpty, pred_v = kEmpty;
    // Second-level state of the predicted next expansion's neighbours (spilled queries,
    // spill_prefetch: spill-table buckets or bitset words): the SQ8 kernels only, where config 5's
    // 10k-query batch spills almost every query (its 10M ids fit only a few hundred LDS slots at full
    // residency): 10.43 -> 9.76 ms with the bitset.  The f32 shapes rarely spill at their table
    // sizes and measured 0.8 % slower with it (profiles/r03/search_experiments/).
    constexpr bool kSpillPrefetch = kSpace != 0;
    // Register merge (pool_merge, pools of <= 128 entries) in the small-row f32 kernels, whose ef
    // at recall 0.95 is ~70 (SIFT-shaped); the SQ8 / wide-row kernels run ef ~370 and keep their
    // registers for the row pass.
    constexpr bool kRegMerge = kSpace == 0 && kChunks > 0 && kChunks <= 8;
    uint32_t pre_u = kEmpty;
    uint64_t pre_lo = 0ull, pre_hi = 0ull;
    while (ps.cur < ps.size) {
      uint32_t c1 = kEmpty, c2 = kEmpty;
      const uint32_t u = pool_pop<kHelp || kScout>(ps, L, &c1, &c2);
      ++n_expand;
      // scout: this node (its memo row stays until it is read at the screen) and the next two pops as
      // the pool stands now -- once the pool is full: nothing is screened before
      if constexpr (kScout) {
        if (scouting && ps.size == ps.ef) scout_post(sboard, 0, 3, u, c1, c2);
      }
      // helpers present: the request for this node (if any; its memo is read in the distance phase)
      // and requests for the next two expansions as the pool stands now
      uint32_t look = 0u;  // (seq << 2) | slot
      if constexpr (kHelp) {
        if (mine.memo_wave < 0 && (n_expand & 3u) == 1u) {  // (a helper appears at most once)
          const uint32_t hw = help_word(board);
          if ((hw >> 8) != 0u) mine.memo_wave = static_cast<int>(hw >> 8) - 1;
        }
        if (mine.memo_wave >= 0) {
#pragma unroll
          for (int hs = 0; hs < kHelpSlots; ++hs)
            if (mine.node[hs] == u) look = (mine.seq[hs] << 2) | static_cast<uint32_t>(hs);
          mine_request(board, wave, mine, u, c1, c2);
        }
      }
#ifndef ALAYA_FINE_STAMPS
      if (kStamp && vs.spilled) st[5]++;
#endif
      stamp(1);
      uint32_t v;
      if (u == pred) {
        v = pred_v;
#ifndef ALAYA_FINE_STAMPS
        if (kStamp) st[7]++;
#endif
      } else {
        v = adjacency_row(p, static_cast<int>(p.R), u);
      }
      // (adjacency_count, written out: through the helper the SQ8 helper kernels of width 4 come out
      // 8 % longer, DESIGN.md "Round 13")
      const uint64_t endm = ballot(lane < static_cast<int>(p.R) && v == kEmpty);
      const int cnt = endm ? __ffsll(static_cast<unsigned long long>(endm)) - 1 : static_cast<int>(p.R);
      bool act = lane < cnt;
#ifdef ALAYA_FINE_STAMPS
      stamp(2);
#endif
      if (p.dedup_edges) {  // graphs with repeated ids in a row: keep the first occurrence only
        for (int j = 0; j < cnt; ++j) {
          const uint32_t vj = read_lane(v, j);
          if (j < lane && vj == v) act = false;
        }
      }
      if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin<space_tab<kSpace>()>(vs);
      if constexpr (kCheck && space_tab<kSpace>()) {
        // diagnostics (tests/test_sq8_spill.py): the buckets read one expansion ahead must equal the
        // table as it is now; a stale one marks the query's counters
        if (u == pre_u && vs.spilled && vs.stab != nullptr) {
          stab_order();
          uint32_t home, code;
          stab_key(vs, v, home, code);
          uint64_t lo2 = 0ull, hi2 = 0ull;
          if (act) stab_load(vs, home, lo2, hi2);
          if (ballot(act && (lo2 != pre_lo || hi2 != pre_hi))) n_hops_up |= 0x40000000u;
        }
      }
      const bool fresh = visit<space_tab<kSpace>()>(vs, v, act, kSpillPrefetch && u == pre_u, pre_lo, pre_hi);
      if constexpr (kSpillPrefetch) {
        // the pred_v load below must issue after this visit's spill-table stores and bitset atomics:
        // the second-level prefetch's wait for pred_v is its wait for them (vmcnt retires in issue
        // order), so no compiler may move the load above them
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
      }
      // consumed: the prefetched state describes the table only up to this visit's stores, so it
      // is never reused (an expansion without fresh neighbours skips the prefetch below, and the
      // next pop must not take this one for its own); zeroed so it is not live across the
      // distance phase either
      pre_u = kEmpty;
      pre_lo = pre_hi = 0ull;
      const uint64_t fm = ballot(fresh);
      const int nf = __popcll(fm);
      // issue the prefetch only after v is consumed: a use of v behind a younger load would
      // otherwise wait for that load too (vmcnt counts in issue order)
      pred = ps.cur < ps.size ? (L.pi[ps.cur] & kIdMask) : kEmpty;
      if (pred != kEmpty) pred_v = adjacency_row(p, static_cast<int>(p.R), pred, pred_v);
#ifdef ALAYA_FINE_STAMPS
      stamp(5);
#else
      stamp(2);
#endif
      if (nf == 0) continue;
      // compact fresh ids in adjacency order
      const uint32_t slot = __popcll(fm & ((1ull << lane) - 1ull));
      if (fresh) L.cid[slot] = v;
      // distances a helper already computed for this node's row (exact: the same function of the same
      // query and row) go straight to cd; the rest are computed here, the known ones standing in the
      // list as kEmpty (distance functions skip them)
      bool memo_ok = false;
      if constexpr (kScout) {
        if (scouting && ps.size == ps.ef && p.screen == 3) memo_ok = scout_lookup(sboard, qi + 1u, u, fresh, slot, L.cd);
      }
      const uint32_t *dist_ids = L.cid;
      bool compute = true;
      if constexpr (kHelp) {
        if (look != 0u) {
          const uint32_t seq = look >> 2;
          const int hs = static_cast<int>(look & 3u);
          const uint64_t *memo = help_memo<kSpace>(p, smem, mine.memo_wave) +
                                 (static_cast<uint32_t>(wave) * kHelpSlots + hs) * p.R;
          uint64_t e = 0ull;
          if (fresh) e = __hip_atomic_load(memo + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          const bool got = fresh && static_cast<uint32_t>(e >> 32) == seq;
          help_retire(board, wave, hs, seq);
          uint32_t *ids2 = reinterpret_cast<uint32_t *>(L.sd);  // free until the merge
          if (fresh) {
            ids2[slot] = got ? kEmpty : v;
            if (got) L.cd[slot] = __uint_as_float(static_cast<uint32_t>(e));
          }
          dist_ids = ids2;
          const uint32_t n_got = __popcll(ballot(got));
          help_count(board, wave, n_got, static_cast<uint32_t>(nf), lane);
          compute = n_got < static_cast<uint32_t>(nf);
        }
      }
      wave_sync();
      // The second-level prefetch of the predicted next expansion goes out right after this
      // expansion's first row pass is issued, so its latency overlaps the rows'.  It needs pred_v,
      // which was loaded after this visit's stores and atomics (the barrier after the visit pins
      // that order) and before the rows: the wait for pred_v (vmcnt counts loads, stores and atomics
      // in issue order) is the wait for them too, so the prefetch reads the table as this visit left
      // it (ALAYA_SPILL_FLAGS bit 8 checks every prefetched bucket against a re-read).
      auto second_level_prefetch = [&]() {
        if constexpr (kSpillPrefetch) {
          if (vs.spilled && pred != kEmpty && !(p.spill_flags & 1u)) {
            if (p.spill_flags & 4u) __builtin_amdgcn_s_waitcnt(0);  // diagnostics: also wait for the rows
            spill_prefetch(vs, pred_v, lane < static_cast<int>(p.R), pre_lo, pre_hi);
            pre_u = pred;
          }
        }
      };
      // Screen (kMode 16).  With the pool full, tau = its worst distance now is >= its worst distance
      // at every later point of the sequential LinearPool::insert order, so a candidate whose exact
      // distance is >= tau is rejected by the reference ("full and d >= last") and changes nothing:
      // not the pool, not cur, not on_next.  One pass over the copies (f16 rows or 8-bit records,
      // p.screen) of all nf rows gives d~;
      // a candidate whose proven lower bound on the exact f32 distance (screen_bound.h) reaches tau
      // is dropped from the list here -- it stays visited and stays counted in n_dist, as in the
      // reference -- and only the others, still in adjacency order, read their f32 rows below, so
      // every distance that can enter the pool has the bits it always had.
      int nd = nf;  // candidates whose f32 row is read
      if constexpr (kScreen) {
        if (ps.size == ps.ef) {
          const float tau = L.pd[ps.size - 1];
          const bool in = lane < nf;
          const uint32_t c = in ? L.cid[lane] : 0u;
          float e_row = 0.f;
          float lb3 = 0.f;  // p.screen == 3: the bound itself
          if (p.screen == 3 && kScout && memo_ok) {  // wave-uniform: the scout's bounds (written to cd above)
            lb3 = L.cd[lane];  // (past the list: a stale word, a bound nobody reads)
            scout_count_screen(sboard, true);
            if (p.scout & kScoutVerify) {  // diagnostics: the searcher's own bounds must have the same bits
              const uint8_t *rp = p.screen_u8 + static_cast<uint64_t>(c) * screen_u8_record_bytes(p.stride);
              const float4 head = *reinterpret_cast<const float4 *>(rp);
              const uint2 sums = *reinterpret_cast<const uint2 *>(rp + screen_u8_sums_offset(p.stride));
              wave_sync();  // (every lane has read its memo bound from cd)
              screen_dots_int<kChunks>(p, sq.codes, L.cid, nf, reinterpret_cast<uint32_t *>(L.cd), NoHook());
              const float own = screen_int_bound(p.stride, sq.err, sq.lo, sq.scale, sq.a1, sq.a2, head.x, head.y, head.z,
                                                 sums.x, sums.y, __float_as_uint(L.cd[lane]));
              const uint32_t bad = static_cast<uint32_t>(__popcll(ballot(in && __float_as_uint(own) != __float_as_uint(lb3))));
              scout_count_mismatches(sboard, bad, lane);
            }
          } else if (p.screen == 3) {  // wave-uniform: the 8-bit records under the integer dot product
            if constexpr (kScout) {
              if (scouting) scout_count_screen(sboard, false);
            }
            // The lane's record header and code sums go out ahead of the pass's loads, in straight-line
            // code (a lane past the list reads row 0's): under `if (in)` the compiler joined this block
            // with the bound's and waited for both loads, two round trips, before the pass was issued.
            const uint8_t *rp = p.screen_u8 + static_cast<uint64_t>(c) * screen_u8_record_bytes(p.stride);
            const float4 head = *reinterpret_cast<const float4 *>(rp);
            const uint2 sums = *reinterpret_cast<const uint2 *>(rp + screen_u8_sums_offset(p.stride));
            screen_dots_int<kChunks>(p, sq.codes, L.cid, nf, reinterpret_cast<uint32_t *>(L.cd), second_level_prefetch);
            lb3 = screen_int_bound(p.stride, sq.err, sq.lo, sq.scale, sq.a1, sq.a2, head.x, head.y, head.z, sums.x, sums.y,
                                   __float_as_uint(L.cd[lane]));  // (past the list: a stale word, a bound nobody reads)
          } else if (p.screen == 2) {  // the 8-bit records in f32 arithmetic, e_row in the header of each
            if (in) e_row = *reinterpret_cast<const float *>(p.screen_u8 + static_cast<uint64_t>(c) * screen_u8_record_bytes(p.stride));
            screen_distances_u8<kChunks, kScreenRowsU8>(p, L.q, L.cid, nf, L.cd, second_level_prefetch);
          } else {
            if (in) e_row = p.screen_err[c];
            screen_distances<kChunks, kScreenRows>(p, L.q, L.cid, nf, L.cd, second_level_prefetch);
          }
          bool keep = false;
          if (in) {
            const float lb = p.screen == 3 ? lb3 : screen_lower_bound(L.cd[lane], e_row, p.dim);
            keep = !(lb > 0.f && lb >= tau);  // lb == 0: no bound (never screened out)
          }
          const uint64_t km = ballot(keep);
          nd = __popcll(km);
          n_screened += static_cast<uint32_t>(nf);
          n_screened_out += static_cast<uint32_t>(nf - nd);
          if constexpr (kScout) {
            if (early && nd > 0 && ps.cur < ps.size) scout_early_request(sboard, L, ps, keep, lb3, c, pred);
          }
          // (every lane read its id before screen_distances' closing wave_sync)
          if (keep) L.cid[__popcll(km & ((1ull << lane) - 1ull))] = c;
          wave_sync();
          if (nd == 0) {
            stamp(3);
            n_dist += nf;
            continue;
          }
        }
      }
      if constexpr (kScreen) {
        // few survivors: a pass of one or two rows per lane group issues no more chunks than it needs
        constexpr int kFull = RowPass<kChunks, kRows>::kR;
        if (nd <= 8) {
          space_distances<kIP, kChunks, kSpace, false, 1>(p, L, L.cid, nd, L.cd);
        } else if (kFull > 2 && nd <= 16) {
          space_distances<kIP, kChunks, kSpace, false, 2>(p, L, L.cid, nd, L.cd);
        } else {  // (the second-level prefetch hook is empty for f32 rows)
          space_distances<kIP, kChunks, kSpace, false, kRows>(p, L, L.cid, nd, L.cd);
        }
      } else if (!kHelp || compute) {
        space_distances<kIP, kChunks, kSpace, kHelp, kRows>(p, L, dist_ids, nf, L.cd, second_level_prefetch);
      } else {
        second_level_prefetch();
      }
      stamp(3);
      n_dist += nf;
      const bool has = lane < nd;
      const uint32_t cid = has ? L.cid[lane] : 0u;
      const float cd = has ? L.cd[lane] : 0.f;
      wave_sync();
      // the merge reports the next pop when it is a newcomer: load its adjacency row while the
      // rest of the merge and the pop run (the prediction above is then stale)
      pool_merge<kRegMerge>(ps, L, has, cid, cd, [&](uint32_t nx) {
        if (nx != pred) {
          const uint32_t old_pred = pred;
          (void)old_pred;
          pred = nx;
          // (adjacency_row, written out: through the helper a kernel-argument load of <30, 16> moves)
          if (lane < static_cast<int>(p.R)) pred_v = p.l0[static_cast<uint64_t>(nx) * p.R + lane];
          if constexpr (kHelp) {  // the new next pop, keeping the old one's request (likely the one after)
            if (mine.memo_wave >= 0) mine_request(board, wave, mine, kEmpty, nx, old_pred);
          }
          if constexpr (kScout) {  // the same for the scout
            if (scouting && ps.size == ps.ef) scout_retarget(sboard, early, nx, old_pred);
          }
        }
      }
#ifdef ALAYA_FINE_STAMPS
      , [&]() { stamp(7); }
#endif
      );
      stamp(4);
    }

    query_end(p, L, ps, qi, n_dist, n_expand, n_dist_up, n_hops_up);
    visit_end(vs);
    if constexpr (kStamp) {
      st[6] = __builtin_readcyclecounter() - t_begin;
      if (lane < 8) p.stamps[static_cast<uint64_t>(qi) * 8 + lane] = st[lane & 7];
    }
    wave_sync();
  }
  if constexpr (kHelp) {
    help_siblings<kIP, kChunks, kSpace>(p, smem, L, board, wave, W);
    help_stats_out(p, board, wave, slot, lane);
  }
  if constexpr (kScout) {
    if (scouting) scout_leave(p, sboard, slot);
  }
  if constexpr (kScreen) screen_stats_out(p, slot, n_screened, n_screened_out, lane);
}

// The screening copy of the base (launch_screen_rows): one wave per row.  err = an over-estimate of
// ||x - f16(x)||_2: the f32 sum of squared differences is at least (1 - (stride + 2) u) of the exact
// one minus the underflow of tiny squares (<= 2 stride 2^-126), so it is scaled up by the bound's
// slack (screen_gamma), its root by 1 + 2^-19 (the sqrt's and the products' roundings), and 2^-50
// covers the root of the underflow.  A row with an element that f16 cannot hold as a finite value
// gets +inf and is never screened out.
__global__ void __launch_bounds__(256) screen_rows_kernel(const float *base, uint64_t first, uint64_t count,
                                                          uint32_t stride, uint16_t *out_rows, float *out_err) {
  const int lane = lane_id();
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); r < count; r += waves) {
    const float *row = base + (first + r) * stride;
    uint16_t *dst = out_rows + (first + r) * stride;
    float sum = 0.f;
    bool bad = false;
    for (uint32_t e = 2 * lane; e < stride; e += 128) {  // stride is a multiple of 32
      const float2 x = *reinterpret_cast<const float2 *>(row + e);
      const _Float16 h0 = static_cast<_Float16>(x.x), h1 = static_cast<_Float16>(x.y);  // round to nearest even
      const float y0 = static_cast<float>(h0), y1 = static_cast<float>(h1);
      bad = bad || !(fabsf(y0) <= 65504.f) || !(fabsf(y1) <= 65504.f) || !(fabsf(x.x) <= FLT_MAX) ||
            !(fabsf(x.y) <= FLT_MAX);
      const float d0 = x.x - y0, d1 = x.y - y1;
      sum = fmaf(d0, d0, sum);
      sum = fmaf(d1, d1, sum);
      const half2_t h = {h0, h1};
      *reinterpret_cast<uint32_t *>(dst + e) = __builtin_bit_cast(uint32_t, h);
    }
    sum += lane_xor<1>(sum);
    sum += lane_xor<2>(sum);
    sum += lane_xor<4>(sum);
    sum += lane_xor<8>(sum);
    sum += lane_xor<16>(sum);
    sum = read_lane(sum, 0) + read_lane(sum, 32);
    const bool any_bad = ballot(bad) != 0ull;
    if (lane == 0) {
      float err = sqrtf(sum * (1.0f + screen_gamma(stride))) * (1.0f + 1.9073486328125e-6f) + 8.8817841970012523e-16f;
      if (any_bad || !(err <= kScreenHuge)) err = __builtin_inff();
      out_err[first + r] = err;
    }
  }
}

// The 8-bit screening copy (launch_screen_rows_u8; record layout, quantiser and e_row in
// screen_bound.h): one wave per row, lane l takes elements 4 l + 256 k.  First the row's min and max,
// then its codes and the f32 sum of (x_j - y_j)^2 over the values the codes stand for.
__global__ void __launch_bounds__(256) screen_rows_u8_kernel(const float *base, uint64_t first, uint64_t count,
                                                             uint32_t stride, uint8_t *out_recs) {
  const int lane = lane_id();
  const uint32_t rec = screen_u8_record_bytes(stride);
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); r < count; r += waves) {
    const float *row = base + (first + r) * stride;
    uint8_t *dst = out_recs + (first + r) * rec;
    float lo = FLT_MAX, hi = -FLT_MAX;
    bool bad = false;
    for (uint32_t e = 4 * lane; e < stride; e += 256) {  // stride is a multiple of 32
      const float4 x = *reinterpret_cast<const float4 *>(row + e);
      bad = bad || !screen_finite(x.x) || !screen_finite(x.y) || !screen_finite(x.z) || !screen_finite(x.w);
      lo = fminf(fminf(lo, x.x), fminf(fminf(x.y, x.z), x.w));
      hi = fmaxf(fmaxf(hi, x.x), fmaxf(fmaxf(x.y, x.z), x.w));
    }
    lo = fminf(lo, lane_xor<1>(lo)); hi = fmaxf(hi, lane_xor<1>(hi));
    lo = fminf(lo, lane_xor<2>(lo)); hi = fmaxf(hi, lane_xor<2>(hi));
    lo = fminf(lo, lane_xor<4>(lo)); hi = fmaxf(hi, lane_xor<4>(hi));
    lo = fminf(lo, lane_xor<8>(lo)); hi = fmaxf(hi, lane_xor<8>(hi));
    lo = fminf(lo, lane_xor<16>(lo)); hi = fmaxf(hi, lane_xor<16>(hi));
    lo = fminf(read_lane(lo, 0), read_lane(lo, 32));
    hi = fmaxf(read_lane(hi, 0), read_lane(hi, 32));
    float scale = screen_u8_scale(lo, hi);
    if (ballot(bad) != 0ull || !screen_finite(scale)) {  // (hi - lo can overflow); codes 0 stand for 0
      bad = true;
      lo = scale = 0.f;
    }
    float sum = 0.f;
    uint32_t s1 = 0u, s2 = 0u;  // sum c, sum c^2: the integer screen's C1, C2
    for (uint32_t e = 4 * lane; e < stride; e += 256) {
      const float4 x = *reinterpret_cast<const float4 *>(row + e);
      const uint32_t c0 = screen_u8_code(x.x, lo, scale), c1 = screen_u8_code(x.y, lo, scale);
      const uint32_t c2 = screen_u8_code(x.z, lo, scale), c3 = screen_u8_code(x.w, lo, scale);
      s1 += (c0 + c1) + (c2 + c3);
      s2 += (c0 * c0 + c1 * c1) + (c2 * c2 + c3 * c3);
      const float d0 = x.x - screen_u8_value(c0, lo, scale), d1 = x.y - screen_u8_value(c1, lo, scale);
      const float d2 = x.z - screen_u8_value(c2, lo, scale), d3 = x.w - screen_u8_value(c3, lo, scale);
      if (!bad) {
        sum = fmaf(d0, d0, sum);
        sum = fmaf(d1, d1, sum);
        sum = fmaf(d2, d2, sum);
        sum = fmaf(d3, d3, sum);
      }
      *reinterpret_cast<uint32_t *>(dst + kScreenU8Header + e) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    }
    sum += lane_xor<1>(sum);
    sum += lane_xor<2>(sum);
    sum += lane_xor<4>(sum);
    sum += lane_xor<8>(sum);
    sum += lane_xor<16>(sum);
    sum = read_lane(sum, 0) + read_lane(sum, 32);
    s1 += lane_xor<1>(s1); s2 += lane_xor<1>(s2);
    s1 += lane_xor<2>(s1); s2 += lane_xor<2>(s2);
    s1 += lane_xor<4>(s1); s2 += lane_xor<4>(s2);
    s1 += lane_xor<8>(s1); s2 += lane_xor<8>(s2);
    s1 += lane_xor<16>(s1); s2 += lane_xor<16>(s2);
    s1 = read_lane(s1, 0) + read_lane(s1, 32);
    s2 = read_lane(s2, 0) + read_lane(s2, 32);
    if (lane == 0) {
      *reinterpret_cast<float4 *>(dst) = make_float4(screen_u8_err(sum, stride, bad), lo, scale, 0.f);
      // in the record's padding (screen_u8_record_bytes: stride is a multiple of 32, so 16 or 48 bytes)
      *reinterpret_cast<uint2 *>(dst + screen_u8_sums_offset(stride)) = make_uint2(s1, s2);
    }
  }
}

// Plain batched distance kernel (one query, list of ids) -- used by the rerank and by tests.
template <bool kIP>
__global__ void __launch_bounds__(64) row_distance_kernel(SearchParams p, const uint32_t *ids,
                                                          uint32_t n, float *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *q = reinterpret_cast<float *>(smem);
  uint32_t *lid = reinterpret_cast<uint32_t *>(smem + static_cast<size_t>(p.stride) * 4);
  float *ld = reinterpret_cast<float *>(lid + 64);
  const int lane = lane_id();
  const float *qsrc = p.queries + static_cast<uint64_t>(blockIdx.y) * p.q_stride;
  for (uint32_t e = lane; e < p.stride; e += 64) q[e] = e < p.dim ? qsrc[e] : 0.f;
  wave_sync();
  for (uint32_t b = blockIdx.x * 64; b < n; b += gridDim.x * 64) {
    const uint32_t cnt = min(64u, n - b);
    if (static_cast<uint32_t>(lane) < cnt) lid[lane] = ids[b + lane];
    wave_sync();
    for (uint32_t c = 0; c < cnt; c += 8)
      row_distances<kIP, 0>(p, q, lid + c, min(8u, cnt - c), ld + c);
    if (static_cast<uint32_t>(lane) < cnt)
      out[static_cast<uint64_t>(blockIdx.y) * n + b + lane] = ld[lane];
    wave_sync();
  }
}


// PyIndex::rerank (python/include/index.hpp:450-488) for SQ8 indexes, Linux batch path (:337-345):
// res_pool[i] holds the k ids the search wrote plus ef-k zeros; all ef entries are rescored with
// the raw-space QueryComputer (f32 rows, FLT_MAX for invalid rows) and the k smallest
// pair<dist, id> are returned (id 0 can repeat -- reference behaviour).  The ef-k zero entries
// are one rescored entry of multiplicity rp.zeros.  Corrected mode (SURVEY A12 "corrected mode
// behind a flag") hands over the whole ef pool with no zeros; shard mode keeps the zeros only on
// the shard holding global row 0 (RerankParams).  kEmpty ids (slots past a pool) are skipped.
// One wave per query.
template <bool kIP>
__global__ void __launch_bounds__(64) rerank_kernel(SearchParams p, RerankParams rp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *q = reinterpret_cast<float *>(smem);
  uint32_t *cid = reinterpret_cast<uint32_t *>(smem + static_cast<size_t>(p.stride) * 4);
  const uint32_t cap = max(rp.k, rp.n_src) + 1;
  float *cd = reinterpret_cast<float *>(cid + cap);
  uint32_t *cm = reinterpret_cast<uint32_t *>(cd + cap);
  const int lane = lane_id();
  const uint32_t taken = rp.n_take;
  const uint32_t zeros = rp.zeros;
  const uint32_t c = taken + (zeros ? 1u : 0u);
  const float fill_d = rp.fill_id == kEmpty ? FLT_MAX : 0.f;
  for (uint64_t qi = blockIdx.x; qi < p.nq; qi += gridDim.x) {
    const float *qsrc = p.queries + qi * p.q_stride;
    for (uint32_t e = lane; e < p.stride; e += 64) q[e] = e < p.dim ? qsrc[e] : 0.f;
    uint32_t nv = 0;  // entries that will be emitted (with multiplicity)
    for (uint32_t b = 0; b < c; b += 64) {
      const uint32_t i = b + lane;
      uint32_t id = 0, m = 0;
      if (i < c) {
        id = i < taken ? rp.search_ids[qi * rp.n_src + i] : 0u;
        m = i < taken ? 1u : zeros;
        if (id == kEmpty) {  // a slot past the pool
          id = 0u;
          m = 0u;
        }
        cid[i] = id;
        cm[i] = m;
      }
      for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
      nv += m;
    }
    wave_sync();
    row_distances<kIP, 0>(p, q, cid, static_cast<int>(c), cd);
    // rank of each distinct entry in the (dist, id) order, equal pairs in entry order
    for (uint32_t i = lane; i < c; i += 64) {
      const float di = cd[i];
      const uint32_t ii = cid[i];
      uint32_t rank = 0;
      for (uint32_t j = 0; j < c; ++j) {
        const float dj = cd[j];
        const uint32_t ij = cid[j];
        const bool less = dj < di || (dj == di && ij < ii);
        const bool tie_before = dj == di && ij == ii && j < i;
        if (less || tie_before) rank += cm[j];
      }
      for (uint32_t m = 0; m < cm[i] && rank + m < rp.k; ++m) {
        rp.out_ids[qi * rp.k + rank + m] = ii;
        if (rp.out_dists) rp.out_dists[qi * rp.k + rank + m] = di;
      }
    }
    for (uint32_t i = nv + lane; i < rp.k; i += 64) {  // fewer candidates than k
      rp.out_ids[qi * rp.k + i] = rp.fill_id;
      if (rp.out_dists) rp.out_dists[qi * rp.k + i] = fill_d;
    }
    wave_sync();
  }
}
// Roofline calibration (bench.py's measured peak): streaming reads of n16 16-byte words, summed so
// the loads cannot be dropped.  Shape 0: one dwordx4 per lane per step (a wave reads 1 KB
// contiguous, the grid sweeps the buffer in order); shape 1: four independent dwordx4 per lane,
// grid-stride apart; shape 2: four consecutive dwordx4 per lane (a wave reads 4 KB contiguous).
// alaya_hbm_stream_read reports the best shape.
template <int kShape>
__global__ void __launch_bounds__(256) stream_read_kernel(const float4 *p, uint64_t n16, float *sink) {
  float acc = 0.f;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if constexpr (kShape == 1) {
    for (; i + 3 * stride < n16; i += 4 * stride) {
      const float4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
      acc += (a.x + b.x) + (c.x + d.x) + (a.w + b.w) + (c.w + d.w);
    }
  } else if constexpr (kShape == 2) {
    const uint64_t w = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);  // wave index
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * 4;
    const uint32_t lane = threadIdx.x & 63;
    uint64_t base = w * 256;
    for (; base + 256 <= n16; base += waves * 256) {
      const float4 a = p[base + lane], b = p[base + 64 + lane], c = p[base + 128 + lane], d = p[base + 192 + lane];
      acc += (a.x + b.x) + (c.x + d.x) + (a.w + b.w) + (c.w + d.w);
    }
    i = n16;  // the tail (< 4 KB per wave) is not read: the byte count below excludes nothing material
  }
  for (; i < n16; i += stride) acc += p[i].x;
  if (acc == -1.2345f) *sink = acc;  // never true for the probe's zeroed buffer
}

// --------------------------------------------------------------------------------------------
// Filtered search: the traversal of hnsw_search_kernel's plain searcher (no helpers, screen, scout or two-waves
// mode; f32 rows), plus a second LinearPool of capacity k per wave, the result pool, that is offered
// every (id, distance) the traversal hands to pool.insert -- in that order -- whose row is valid and
// allowed by the query's mask.  The traversal pool, the visited set, every pop and the four counters
// are those of the unfiltered search at the same ef; the output is the result pool, then empty slots
// (kEmpty, FLT_MAX).  The result pool sits at f.result_off of the wave's LDS region, past the visited
// table, so carve_lds and every offset the other kernels use stay as they are.
// --------------------------------------------------------------------------------------------
// The wave's result pool as an Lds whose pool is the result pool (pool_merge's view; sd is shared
// scratch, free between two merges).
__device__ __forceinline__ Lds result_lds(const Lds &L, const FilterParams &f) {
  Lds Lr = L;
  unsigned char *ptr = reinterpret_cast<unsigned char *>(L.q) + f.result_off;
  Lr.pd = reinterpret_cast<float *>(ptr);
  Lr.pi = reinterpret_cast<uint32_t *>(ptr + ((f.k + 1) * 4 + 15) / 16 * 16);
  return Lr;
}

// result.insert(id, d) for the lanes with ok, in lane order.  Most offers find the pool full and every
// distance at or past its worst one: one LDS read and one ballot, no merge.
__device__ __forceinline__ void result_offer(PoolState &rs, const Lds &Lr, bool ok, uint32_t id, float d) {
  const bool full = rs.size == rs.ef;
  const float worst = full ? Lr.pd[rs.size - 1] : 0.f;
  if (ballot(ok && !(full && d >= worst)) == 0ull) return;
  pool_merge(rs, Lr, ok, id, d);
}

template <bool kIP, int kChunks>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(search_min_waves<kChunks, 0, 0>() ? search_min_waves<kChunks, 0, 0>() : 1, 8)))
    filtered_search_kernel(SearchParams p, FilterParams f) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kSpace = 0;
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x >> 6);
  const int W = static_cast<int>(blockDim.x >> 6);
  const Lds L = carve_lds<kSpace>(p, smem, wave);
  const Lds Lr = result_lds(L, f);
  const uint64_t bit_words = (p.n + 31) / 32;
  const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * W + wave;
  uint32_t *slot_bits = p.overflow_bits + slot * bit_words;
  uint32_t *slot_dirty = p.dirty_words + slot * p.dirty_cap;
  constexpr bool kRegMerge = kChunks > 0 && kChunks <= 8;  // as the plain kernel's traversal merge

  for (;;) {
    uint32_t qi = 0;
    if (lane == 0) qi = atomicAdd(p.work_counter, 1u);
    qi = read_lane(qi, 0);
    if (qi >= p.nq) break;
    // the query's mask; a row is allowed if its bit is set and (indexes with a bitmap) it is valid
    const uint32_t *mask = f.allow + static_cast<uint64_t>(f.mask_of_query != nullptr ? f.mask_of_query[qi] : 0u) * f.mask_words;
    for (uint32_t e = lane; e <= f.k; e += 64) {
      Lr.pd[e] = 0.f;
      Lr.pi[e] = 0u;
    }
    PoolState rs{0u, 0u, f.k};
    Visited vs;
    PoolState ps;
    uint32_t n_dist = 0, n_expand = 0, n_dist_up = 0, n_hops_up = 0;
    // (query_begin's first wave_sync orders the reset above before any offer)
    query_begin<kIP, kChunks, kSpace>(p, L, qi, slot_bits, slot_dirty, nullptr, vs, ps, n_dist_up, n_hops_up,
                                      [&](bool has, uint32_t id, float d) {
                                        bool ok = false;
                                        if (has) {
                                          ok = ((mask[id >> 5] >> (id & 31)) & 1u) != 0u;
                                          if (p.valid != nullptr) ok = ok && ((p.valid[id >> 5] >> (id & 31)) & 1u) != 0u;
                                        }
                                        result_offer(rs, Lr, ok, id, d);
                                      });

    // ---- best-first expansion: the plain searcher's loop ------------------------------------
    uint32_t pred = kEmpty, pred_v = kEmpty;  // adjacency prefetch of the predicted next pop
    while (ps.cur < ps.size) {
      const uint32_t u = pool_pop(ps, L);
      ++n_expand;
      uint32_t v = u == pred ? pred_v : adjacency_row(p, static_cast<int>(p.R), u);
      const int cnt = adjacency_count(static_cast<int>(p.R), v);
      bool act = lane < cnt;
      if (p.dedup_edges) {  // graphs with repeated ids in a row: keep the first occurrence only
        for (int j = 0; j < cnt; ++j) {
          const uint32_t vj = read_lane(v, j);
          if (j < lane && vj == v) act = false;
        }
      }
      if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin(vs);
      const bool fresh = visit(vs, v, act);
      const uint64_t fm = ballot(fresh);
      const int nf = __popcll(fm);
      pred = ps.cur < ps.size ? (L.pi[ps.cur] & kIdMask) : kEmpty;
      if (pred != kEmpty) pred_v = adjacency_row(p, static_cast<int>(p.R), pred, pred_v);
      if (nf == 0) continue;
      // compact fresh ids in adjacency order
      if (fresh) L.cid[__popcll(fm & ((1ull << lane) - 1ull))] = v;
      wave_sync();
      // The candidates are known: each one's allow word (and validity word) goes out here, ahead of
      // the row gather, by the lane that will hold the candidate at the merges; the words are used
      // only after the distances, so their latency is the rows'.
      const bool has = lane < nf;
      const uint32_t cid = has ? L.cid[lane] : 0u;
      uint32_t aw = 0u, vw = 0xffffffffu;
      if (has) {
        aw = mask[cid >> 5];
        if (p.valid != nullptr) vw = p.valid[cid >> 5];
      }
      space_distances<kIP, kChunks, kSpace>(p, L, L.cid, nf, L.cd);
      n_dist += nf;
      const float cd = has ? L.cd[lane] : 0.f;
      wave_sync();
      pool_merge<kRegMerge>(ps, L, has, cid, cd, [&](uint32_t nx) {
        if (nx != pred) {
          pred = nx;
          pred_v = adjacency_row(p, static_cast<int>(p.R), nx, pred_v);
        }
      });
      result_offer(rs, Lr, has && (((aw & vw) >> (cid & 31)) & 1u) != 0u, cid, cd);
    }

    query_end(p, Lr, rs, qi, n_dist, n_expand, n_dist_up, n_hops_up);
    visit_end(vs);
    wave_sync();
  }
}
}  // namespace

hipError_t launch_stream_read(const void *buf, uint64_t bytes, int grid, int shape, float *sink,
                              hipStream_t stream) {
  const float4 *p = static_cast<const float4 *>(buf);
  if (shape == 1) {
    hipLaunchKernelGGL(stream_read_kernel<1>, dim3(grid), dim3(256), 0, stream, p, bytes / 16, sink);
  } else if (shape == 2) {
    hipLaunchKernelGGL(stream_read_kernel<2>, dim3(grid), dim3(256), 0, stream, p, bytes / 16, sink);
  } else {
    hipLaunchKernelGGL(stream_read_kernel<0>, dim3(grid), dim3(256), 0, stream, p, bytes / 16, sink);
  }
  return hipGetLastError();
}

size_t search_query_lds_bytes(uint32_t stride, int sq8_order) {
  // the query as f32 terms, or (ALAYA_SQ8_QCODES, AVX-512-order SQ8) as its codes, 16 B aligned
  return sq8_order == 2 && sq8_query_codes<2>() ? (static_cast<size_t>(stride) + 15) / 16 * 16
                                                : static_cast<size_t>(stride) * 4;
}

size_t search_wave_lds_bytes(uint32_t stride, uint32_t ef, uint32_t hash_log2, bool compact, int sq8_order) {
  return search_query_lds_bytes(stride, sq8_order) + 3 * 64 * 4 + 2 * (((ef + 1) * 4 + 15) / 16 * 16) +
         visited_table_bytes(hash_log2, compact);
}

hipError_t launch_rerank(const SearchParams &p, const RerankParams &r, hipStream_t stream) {
  const size_t lds = static_cast<size_t>(p.stride) * 4 + 3 * (static_cast<size_t>(std::max(r.k, r.n_src)) + 1) * 4 + 64;
  const int grid = static_cast<int>(std::min<uint64_t>(p.nq, 4096));
  if (p.ip) {
    hipLaunchKernelGGL(rerank_kernel<true>, dim3(grid), dim3(64), lds, stream, p, r);
  } else {
    hipLaunchKernelGGL(rerank_kernel<false>, dim3(grid), dim3(64), lds, stream, p, r);
  }
  return hipGetLastError();
}

template <bool kIP, int kChunks, int kMode, int kSpace>
static const void *kernel_ptr() {
  return reinterpret_cast<const void *>(&hnsw_search_kernel<kIP, kChunks, kMode, kSpace>);
}

// The kernels of search_variants.h's list, row for row.
struct SearchKernels {
  const void *ip, *l2;
};
#define ALAYA_IP_both(S, C, M) kernel_ptr<true, C, M, S>()
#define ALAYA_IP_l2(S, C, M) nullptr
#define ALAYA_KERNEL_ROW(S, C, M, METRICS) {ALAYA_IP_##METRICS(S, C, M), kernel_ptr<false, C, M, S>()},
static const SearchKernels kSearchKernels[] = {ALAYA_SEARCH_VARIANTS(ALAYA_KERNEL_ROW)};
#undef ALAYA_KERNEL_ROW
static_assert(sizeof(kSearchKernels) / sizeof(kSearchKernels[0]) == kNumSearchVariants, "one kernel row per variant");

static const void *search_kernel_symbol(const SearchVariant &v, bool ip) {
  const SearchKernels &k = kSearchKernels[&v - kSearchVariants];
  return ip ? k.ip : k.l2;
}

hipError_t launch_screen_rows(const float *base, uint64_t first, uint64_t count, uint32_t stride,
                              uint16_t *out_rows, float *out_err, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const int grid = static_cast<int>(std::min<uint64_t>((count + 3) / 4, 16384));
  hipLaunchKernelGGL(screen_rows_kernel, dim3(grid), dim3(256), 0, stream, base, first, count, stride, out_rows,
                     out_err);
  return hipGetLastError();
}

hipError_t launch_screen_rows_u8(const float *base, uint64_t first, uint64_t count, uint32_t stride,
                                 uint8_t *out_recs, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const int grid = static_cast<int>(std::min<uint64_t>((count + 3) / 4, 16384));
  hipLaunchKernelGGL(screen_rows_u8_kernel, dim3(grid), dim3(256), 0, stream, base, first, count, stride, out_recs);
  return hipGetLastError();
}

hipError_t launch_search(const SearchVariant &v, const SearchParams &p, int grid, int waves, size_t lds,
                         hipStream_t stream) {
  SearchParams arg = p;
  void *args[] = {&arg};
  return hipLaunchKernel(search_kernel_symbol(v, p.ip), dim3(grid), dim3(64 * waves), args, lds, stream);
}

hipError_t launch_row_distances(const SearchParams &p, const uint32_t *ids, uint32_t n,
                                uint32_t nq, float *out, hipStream_t stream) {
  const size_t lds = static_cast<size_t>(p.stride) * 4 + 128 * 4;
  const int gx = static_cast<int>(std::min<uint32_t>((n + 63) / 64, 1024u));
  if (p.ip) {
    hipLaunchKernelGGL(row_distance_kernel<true>, dim3(gx, nq), dim3(64), lds, stream, p, ids, n, out);
  } else {
    hipLaunchKernelGGL(row_distance_kernel<false>, dim3(gx, nq), dim3(64), lds, stream, p, ids, n, out);
  }
  return hipGetLastError();
}

hipError_t search_occupancy(const SearchVariant &v, bool ip, int waves, size_t lds, int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, search_kernel_symbol(v, ip), 64 * waves, lds);
}

// The filtered kernels: {L2, IP} x the plain f32 kernels' widths; the generic element order rides on
// the runtime-d kernel (chunks 0), as in the plain kernel.
template <int... kChunks>
static const void *filtered_symbol_of(int chunks, bool ip) {
  const void *sym = nullptr;
  ((chunks == kChunks ? (sym = ip ? reinterpret_cast<const void *>(&filtered_search_kernel<true, kChunks>)
                                  : reinterpret_cast<const void *>(&filtered_search_kernel<false, kChunks>),
                         0)
                      : 0),
   ...);
  return sym;
}

static const void *filtered_kernel_symbol(uint32_t dim, bool generic, bool ip) {
  const void *sym = filtered_symbol_of<4, 8, 16, 24, 30, 32>(search_chunks(dim, generic), ip);
  return sym != nullptr ? sym : filtered_symbol_of<0>(0, ip);
}

size_t filter_result_lds_bytes(uint32_t k) { return 2 * ((static_cast<size_t>(k + 1) * 4 + 15) / 16 * 16); }

hipError_t launch_filtered_search(const SearchParams &p, const FilterParams &f, int grid, int waves, size_t lds,
                                  hipStream_t stream) {
  SearchParams arg = p;
  FilterParams farg = f;
  void *args[] = {&arg, &farg};
  return hipLaunchKernel(filtered_kernel_symbol(p.dim, p.generic, p.ip), dim3(grid), dim3(64 * waves), args, lds, stream);
}

hipError_t filtered_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, filtered_kernel_symbol(dim, generic, ip), 64 * waves,
                                                      lds);
}

// --------------------------------------------------------------------------------------------
// Filtered search of SQ8 codes: the traversal of hnsw_search_kernel's plain (mode 0) SQ8 searcher -- the
// query encoded to codes, code-to-code distances without a validity test, the spill levels and their
// prefetch -- plus the candidate pool: a second LinearPool of capacity f.k = m per wave that is offered
// every (id, code distance) the traversal hands to pool.insert, in that order, whose row is valid and
// allowed by the query's mask.  The traversal pool, the visited set, every pop and the four counters
// are those of the unfiltered SQ8 search at the same ef.  The output is the candidate pool's ids, then
// kEmpty: launch_rerank rescores them on the f32 rows.  Four waves per workgroup share the quantizer's
// scale / min; they meet once, in fill_shared, before any wave draws a query.  The candidate pool sits
// at f.result_off of the wave's LDS region, past the visited table (carve_lds is unchanged).
// --------------------------------------------------------------------------------------------
namespace {
// candidates.insert(id, d) for the lanes with `allowed`, in lane order: result_offer with the validity bitmap
// read last, and only when some allowed lane's distance can enter the pool -- rarely once the pool is full --
// so no validity word is live across the distance pass of a kernel that is at its register budget.
// (Dropping the lanes that `full && d >= worst` rejects before the merge changes nothing: the merge rejects
// them by the same test.)
__device__ __forceinline__ void candidate_offer(const SearchParams &p, PoolState &rs, const Lds &Lr, bool allowed, uint32_t id,
                                                float d) {
  const bool full = rs.size == rs.ef;
  const float worst = full ? Lr.pd[rs.size - 1] : 0.f;
  bool ok = allowed && !(full && d >= worst);
  if (ballot(ok) == 0ull) return;
  if (p.valid != nullptr && ok) ok = ((p.valid[id >> 5] >> (id & 31)) & 1u) != 0u;
  pool_merge(rs, Lr, ok, id, d);
}

template <bool kIP, int kChunks, int kSpace>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(search_min_waves<kChunks, kSpace, 0>() ? search_min_waves<kChunks, kSpace, 0>() : 1, 8)))
    filtered_sq8_search_kernel(SearchParams p, FilterParams f) {
  static_assert(space_sq8<kSpace>(), "SQ8 codes");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool kTab = space_tab<kSpace>();
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x >> 6);
  const int W = static_cast<int>(blockDim.x >> 6);
  const Lds L = carve_lds<kSpace>(p, smem, wave);
  fill_shared<kSpace>(p, L);  // the workgroup's only barrier: every wave passes it, with or without a query
  const Lds Lr = result_lds(L, f);
  const uint64_t bit_words = (p.n + 31) / 32;
  const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * W + wave;
  uint32_t *slot_bits = p.overflow_bits + slot * bit_words;
  uint32_t *slot_dirty = p.dirty_words + slot * p.dirty_cap;
  uint16_t *slot_stab = (kTab && p.spill_table) ? p.spill_table + (slot << p.stab_log2) : nullptr;

  for (;;) {
    uint32_t qi = 0;
    if (lane == 0) qi = atomicAdd(p.work_counter, 1u);
    qi = read_lane(qi, 0);
    if (qi >= p.nq) break;
    // the query's mask; a row is allowed if its bit is set and (indexes with a bitmap) it is valid
    const uint32_t *mask = f.allow + static_cast<uint64_t>(f.mask_of_query != nullptr ? f.mask_of_query[qi] : 0u) * f.mask_words;
    for (uint32_t e = lane; e <= f.k; e += 64) {
      Lr.pd[e] = 0.f;
      Lr.pi[e] = 0u;
    }
    PoolState rs{0u, 0u, f.k};
    Visited vs;
    PoolState ps;
    uint32_t n_dist = 0, n_expand = 0, n_dist_up = 0, n_hops_up = 0;
    // (query_begin's first wave_sync orders the reset above before any offer)
    query_begin<kIP, kChunks, kSpace>(p, L, qi, slot_bits, slot_dirty, slot_stab, vs, ps, n_dist_up, n_hops_up,
                                      [&](bool has, uint32_t id, float d) {
                                        const bool allowed = has && ((mask[id >> 5] >> (id & 31)) & 1u) != 0u;
                                        candidate_offer(p, rs, Lr, allowed, id, d);
                                      });

    // ---- best-first expansion: the plain SQ8 searcher's loop ----------------------------------
    uint32_t pred = kEmpty, pred_v = kEmpty;  // adjacency prefetch of the predicted next pop
    uint32_t pre_u = kEmpty;                  // second-level state read one expansion ahead (spill_prefetch)
    uint64_t pre_lo = 0ull, pre_hi = 0ull;
    while (ps.cur < ps.size) {
      const uint32_t u = pool_pop(ps, L);
      ++n_expand;
      uint32_t v = u == pred ? pred_v : adjacency_row(p, static_cast<int>(p.R), u);
      const int cnt = adjacency_count(static_cast<int>(p.R), v);
      bool act = lane < cnt;
      if (p.dedup_edges) {  // graphs with repeated ids in a row: keep the first occurrence only
        for (int j = 0; j < cnt; ++j) {
          const uint32_t vj = read_lane(v, j);
          if (j < lane && vj == v) act = false;
        }
      }
      if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin<kTab>(vs);
      const bool fresh = visit<kTab>(vs, v, act, u == pre_u, pre_lo, pre_hi);
      // the pred_v load below issues after this visit's spill-table stores and bitset atomics: the
      // second-level prefetch's wait for pred_v is its wait for them (as in hnsw_search_kernel)
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" ::: "memory");
      pre_u = kEmpty;  // consumed: the prefetched state describes the table only up to this visit's stores
      pre_lo = pre_hi = 0ull;
      const uint64_t fm = ballot(fresh);
      const int nf = __popcll(fm);
      pred = ps.cur < ps.size ? (L.pi[ps.cur] & kIdMask) : kEmpty;
      if (pred != kEmpty) pred_v = adjacency_row(p, static_cast<int>(p.R), pred, pred_v);
      if (nf == 0) continue;
      // compact fresh ids in adjacency order
      if (fresh) L.cid[__popcll(fm & ((1ull << lane) - 1ull))] = v;
      wave_sync();
      // each candidate's allow word goes out ahead of the code rows, by the lane that will hold the
      // candidate at the merges; it is used only after the distances, so its latency is the rows'
      const bool has = lane < nf;
      uint32_t aw = 0u;
      if (has) aw = mask[L.cid[lane] >> 5];
      space_distances<kIP, kChunks, kSpace>(p, L, L.cid, nf, L.cd, [&]() {
        // the predicted next expansion's second-level state, behind this expansion's first row pass
        if (vs.spilled && pred != kEmpty && !(p.spill_flags & 1u)) {
          spill_prefetch(vs, pred_v, lane < static_cast<int>(p.R), pre_lo, pre_hi);
          pre_u = pred;
        }
      });
      n_dist += nf;
      const uint32_t cid = has ? L.cid[lane] : 0u;
      const float cd = has ? L.cd[lane] : 0.f;
      wave_sync();
      pool_merge(ps, L, has, cid, cd, [&](uint32_t nx) {
        if (nx != pred) {
          pred = nx;
          pred_v = adjacency_row(p, static_cast<int>(p.R), nx, pred_v);
        }
      });
      candidate_offer(p, rs, Lr, has && ((aw >> (cid & 31)) & 1u) != 0u, cid, cd);
    }

    query_end(p, Lr, rs, qi, n_dist, n_expand, n_dist_up, n_hops_up);
    visit_end(vs);
    wave_sync();
  }
}
}  // namespace

// The filtered SQ8 kernels: {L2, IP} x the code order x the plain SQ8 kernels' widths (the mode-0 SQ8
// rows of search_variants.h); any other width runs the runtime-d kernel (chunks 0).
template <int kSpace, int... kChunks>
static const void *filtered_sq8_symbol_of(int chunks, bool ip) {
  const void *sym = nullptr;
  ((chunks == kChunks ? (sym = ip ? reinterpret_cast<const void *>(&filtered_sq8_search_kernel<true, kChunks, kSpace>)
                                  : reinterpret_cast<const void *>(&filtered_sq8_search_kernel<false, kChunks, kSpace>),
                         0)
                      : 0),
   ...);
  return sym;
}

static const void *filtered_sq8_kernel_symbol(uint32_t dim, int sq8_order, bool ip) {
  const int chunks = search_chunks(dim, false);
  const void *sym = sq8_order == 2 ? filtered_sq8_symbol_of<2, 4, 24, 30>(chunks, ip)
                                   : filtered_sq8_symbol_of<1, 4, 24, 30>(chunks, ip);
  if (sym != nullptr) return sym;
  return sq8_order == 2 ? filtered_sq8_symbol_of<2, 0>(0, ip) : filtered_sq8_symbol_of<1, 0>(0, ip);
}

hipError_t launch_filtered_sq8_search(const SearchParams &p, const FilterParams &f, int grid, int waves, size_t lds,
                                      hipStream_t stream) {
  SearchParams arg = p;
  FilterParams farg = f;
  void *args[] = {&arg, &farg};
  return hipLaunchKernel(filtered_sq8_kernel_symbol(p.dim, p.sq8_order, p.ip), dim3(grid), dim3(64 * waves), args, lds,
                         stream);
}

hipError_t filtered_sq8_search_occupancy(uint32_t dim, int sq8_order, bool ip, int waves, size_t lds,
                                         int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, filtered_sq8_kernel_symbol(dim, sq8_order, ip),
                                                      64 * waves, lds);
}

// --------------------------------------------------------------------------------------------
// Through search: the filtered search with a second expansion rule.  passable(v) = v's allow bit is set
// and (indexes with a bitmap) v is valid.  A popped node's neighbour that is not passable is neither
// measured nor kept: it is marked visited and its own level-0 row is walked instead, one level deep, for
// passable rows not yet visited (a row that is not passable is skipped there without a visited mark).  So
// the traversal pool of ef entries holds passable rows only, beside the entry, which goes in whatever its
// bit.  Per pop: the direct row's passable fresh neighbours, then each through row's, in adjacency order --
// the order of the sequential pool.insert / result.insert calls this kernel equals (include/alaya_hip.h,
// alaya_index_filtered_search_hop).  The candidates queue up in L.cid and are measured and merged 64 at the
// most at a time: a flush.  LDS is the filtered kernel's; the through list is a ballot mask, and the
// adjacency rows of kHopRows through nodes, with their allow bits, are in flight together in registers.
// --------------------------------------------------------------------------------------------
namespace {

constexpr int kHopRows = 8;

// A batch of through rows, one register each, as a queue: the next row is x0, and taking it moves the others
// down.  (Nothing is ever selected by the wave-uniform row index: the compiler turns such a selection into an
// indexed load, which puts the batch in scratch.)
struct HopBatch {
  uint32_t x0, x1, x2, x3, x4, x5, x6, x7;
};
static_assert(sizeof(HopBatch) == kHopRows * 4, "one register per row");

__device__ __forceinline__ uint32_t hop_take(HopBatch &b) {
  const uint32_t r = b.x0;
  b.x0 = b.x1;
  b.x1 = b.x2;
  b.x2 = b.x3;
  b.x3 = b.x4;
  b.x4 = b.x5;
  b.x5 = b.x6;
  b.x6 = b.x7;
  b.x7 = kEmpty;
  return r;
}

// lanes of `m` append their id to the candidate queue, in lane order, behind its qn entries
__device__ __forceinline__ void hop_append(const Lds &L, int qn, uint64_t m, uint32_t id) {
  const int lane = lane_id();
  if ((m >> lane) & 1ull) L.cid[qn + __popcll(m & ((1ull << lane) - 1ull))] = id;
}

template <bool kIP, int kChunks>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(search_min_waves<kChunks, 0, 0>() ? search_min_waves<kChunks, 0, 0>() : 1, 8)))
    filtered_hop_search_kernel(SearchParams p, FilterParams f, HopParams h) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kSpace = 0;
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x >> 6);
  const int W = static_cast<int>(blockDim.x >> 6);
  const int R = static_cast<int>(p.R);
  const Lds L = carve_lds<kSpace>(p, smem, wave);
  const Lds Lr = result_lds(L, f);
  const uint64_t bit_words = (p.n + 31) / 32;
  const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * W + wave;
  uint32_t *slot_bits = p.overflow_bits + slot * bit_words;
  uint32_t *slot_dirty = p.dirty_words + slot * p.dirty_cap;
  constexpr bool kRegMerge = kChunks > 0 && kChunks <= 8;  // as the plain kernel's traversal merge

  for (;;) {
    uint32_t qi = 0;
    if (lane == 0) qi = atomicAdd(p.work_counter, 1u);
    qi = read_lane(qi, 0);
    if (qi >= p.nq) break;
    const uint32_t *mask = f.allow + static_cast<uint64_t>(f.mask_of_query != nullptr ? f.mask_of_query[qi] : 0u) * f.mask_words;
    // the row's allow word, and-ed with its validity word: bit (id & 31) = passable
    auto pass_word = [&](uint32_t id) {
      uint32_t w = mask[id >> 5];
      if (p.valid != nullptr) w &= p.valid[id >> 5];
      return w;
    };
    for (uint32_t e = lane; e <= f.k; e += 64) {
      Lr.pd[e] = 0.f;
      Lr.pi[e] = 0u;
    }
    PoolState rs{0u, 0u, f.k};
    Visited vs;
    PoolState ps;
    uint32_t n_dist = 0, n_expand = 0, n_dist_up = 0, n_hops_up = 0, n_through = 0;
    // (query_begin's first wave_sync orders the reset above before any offer)
    query_begin<kIP, kChunks, kSpace>(p, L, qi, slot_bits, slot_dirty, nullptr, vs, ps, n_dist_up, n_hops_up,
                                      [&](bool has, uint32_t id, float d) {
                                        bool ok = false;
                                        if (has) ok = ((pass_word(id) >> (id & 31)) & 1u) != 0u;
                                        result_offer(rs, Lr, ok, id, d);
                                      });

    uint32_t pred = kEmpty, pred_v = kEmpty;  // adjacency prefetch of the predicted next pop
    while (ps.cur < ps.size) {
      const uint32_t u = pool_pop(ps, L);
      ++n_expand;
      // ---- direct row: the bit decides candidate or through, so its word is read before the visit ----
      const uint32_t v = u == pred ? pred_v : adjacency_row(p, R, u);
      const int cnt = adjacency_count(R, v);
      bool act = lane < cnt;
      if (p.dedup_edges) {  // graphs with repeated ids in a row: keep the first occurrence only
        for (int j = 0; j < cnt; ++j) {
          const uint32_t vj = read_lane(v, j);
          if (j < lane && vj == v) act = false;
        }
      }
      bool pass = false;
      if (act) pass = ((pass_word(v) >> (v & 31)) & 1u) != 0u;
      if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin(vs);
      const bool fresh = visit(vs, v, act);
      const uint64_t fm = ballot(fresh && pass);
      uint64_t rest = ballot(fresh && !pass);  // the through list, adjacency order
      n_through += __popcll(rest);
      int qn = __popcll(fm);                   // candidates queued in L.cid
      pred = ps.cur < ps.size ? (L.pi[ps.cur] & kIdMask) : kEmpty;
      if (pred != kEmpty) pred_v = adjacency_row(p, R, pred, pred_v);
      if (qn == 0 && rest == 0ull) continue;
      hop_append(L, 0, fm, v);

      // ---- through rows, kHopRows at a time: row loads, then their allow words, all in flight ----
      HopBatch x{kEmpty, kEmpty, kEmpty, kEmpty, kEmpty, kEmpty, kEmpty, kEmpty};
      uint32_t okb = 0u;  // bit j: this lane's entry of the batch's row j is passable
      int bn = 0;         // rows left in the batch
      bool pend = false;   // a row whose fresh ids wait for the flush that makes room
      uint32_t px = 0u;
      uint64_t pm = 0ull;
      for (;;) {
        if (pend) {
          hop_append(L, qn, pm, px);
          qn += __popcll(pm);
          pend = false;
        }
        while (rest != 0ull) {
          if (bn == 0) {
            uint64_t r2 = rest;
            // the next through node's row, kEmpty in every lane past the list's end
            auto next_row = [&]() {
              if (r2 == 0ull) return kEmpty;
              const uint32_t w = read_lane(v, __ffsll(static_cast<unsigned long long>(r2)) - 1);
              r2 &= r2 - 1ull;
              ++bn;
              return adjacency_row(p, R, w);
            };
            x.x0 = next_row();
            x.x1 = next_row();
            x.x2 = next_row();
            x.x3 = next_row();
            x.x4 = next_row();
            x.x5 = next_row();
            x.x6 = next_row();
            x.x7 = next_row();
            // (every lane loads, a lane past its row the word of row 0: eight independent gathers, no branch)
            auto pass_bit = [&](uint32_t id) {
              const uint32_t at = id != kEmpty ? id : 0u;
              const uint32_t bit = (pass_word(at) >> (at & 31)) & 1u;
              return id != kEmpty ? bit : 0u;
            };
            okb = pass_bit(x.x0) | pass_bit(x.x1) << 1 | pass_bit(x.x2) << 2 | pass_bit(x.x3) << 3 | pass_bit(x.x4) << 4 |
                  pass_bit(x.x5) << 5 | pass_bit(x.x6) << 6 | pass_bit(x.x7) << 7;
          }
          const uint32_t xr = hop_take(x);
          const bool okr = (okb & 1u) != 0u;
          okb >>= 1;
          --bn;
          rest &= rest - 1ull;
          const int cnt2 = adjacency_count(R, xr);
          bool act2 = lane < cnt2;
          if (p.dedup_edges) {
            for (int j = 0; j < cnt2; ++j) {
              const uint32_t xj = read_lane(xr, j);
              if (j < lane && xj == xr) act2 = false;
            }
          }
          if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin(vs);
          const uint64_t m2 = ballot(visit(vs, xr, act2 && okr));
          if (m2 == 0ull) continue;
          if (qn + __popcll(m2) > 64) {  // no room: flush first
            px = xr;
            pm = m2;
            pend = true;
            break;
          }
          hop_append(L, qn, m2, xr);
          qn += __popcll(m2);
        }
        if (qn == 0) break;
        // ---- flush: distances, traversal merge, result offer (every queued id is passable) ----
        wave_sync();
        const bool has = lane < qn;
        const uint32_t cid = has ? L.cid[lane] : 0u;
        space_distances<kIP, kChunks, kSpace>(p, L, L.cid, qn, L.cd);
        n_dist += qn;
        const float cd = has ? L.cd[lane] : 0.f;
        wave_sync();
        pool_merge<kRegMerge>(ps, L, has, cid, cd, [&](uint32_t nx) {
          if (nx != pred) {
            pred = nx;
            pred_v = adjacency_row(p, R, nx, pred_v);
          }
        });
        result_offer(rs, Lr, has, cid, cd);
        wave_sync();
        qn = 0;
        if (!pend && rest == 0ull) break;
      }
    }

    query_end(p, Lr, rs, qi, n_dist, n_expand, n_dist_up, n_hops_up);
    if (h.n_through != nullptr && lane == 0) h.n_through[qi] = n_through;
    visit_end(vs);
    wave_sync();
  }
}
}  // namespace

// The through kernels: the filtered kernels' set.
template <int... kChunks>
static const void *filtered_hop_symbol_of(int chunks, bool ip) {
  const void *sym = nullptr;
  ((chunks == kChunks ? (sym = ip ? reinterpret_cast<const void *>(&filtered_hop_search_kernel<true, kChunks>)
                                  : reinterpret_cast<const void *>(&filtered_hop_search_kernel<false, kChunks>),
                         0)
                      : 0),
   ...);
  return sym;
}

static const void *filtered_hop_kernel_symbol(uint32_t dim, bool generic, bool ip) {
  const void *sym = filtered_hop_symbol_of<4, 8, 16, 24, 30, 32>(search_chunks(dim, generic), ip);
  return sym != nullptr ? sym : filtered_hop_symbol_of<0>(0, ip);
}

hipError_t launch_filtered_hop_search(const SearchParams &p, const FilterParams &f, const HopParams &h, int grid, int waves,
                                      size_t lds, hipStream_t stream) {
  SearchParams arg = p;
  FilterParams farg = f;
  HopParams harg = h;
  void *args[] = {&arg, &farg, &harg};
  return hipLaunchKernel(filtered_hop_kernel_symbol(p.dim, p.generic, p.ip), dim3(grid), dim3(64 * waves), args, lds,
                         stream);
}

hipError_t filtered_hop_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, filtered_hop_kernel_symbol(dim, generic, ip), 64 * waves,
                                                      lds);
}

// --------------------------------------------------------------------------------------------
// Range search: the filtered search's traversal -- hnsw_search_kernel's plain searcher, f32 rows -- with
// the result pool replaced by an append list cut at a radius.  Every (id, distance) the traversal hands
// to pool.insert, in that order, whose row is valid, allowed by the query's mask (f.allow == nullptr: no
// mask) and has d <= radius is a hit.  The wave counts every hit and stores the first r.cap of them, in
// arrival order, in the query's region of the global append buffers; range_sort_kernel orders them.  The
// traversal pool, the visited set, every pop and the four counters are those of the unfiltered search at
// the same ef.  No LDS beyond the plain searcher's; p.k = 0, so query_end writes the counters only.
// --------------------------------------------------------------------------------------------
namespace {

// The hits among the lanes with ok, appended in lane order behind the query's `count` earlier ones: one
// ballot, each lane's slot from the popcount of the hits below it, stores while the slot is below the cap.
__device__ __forceinline__ void range_offer(uint32_t &count, const RangeParams &r, uint64_t region, float radius, bool ok,
                                            uint32_t id, float d) {
  const bool hit = ok && d <= radius;
  const uint64_t hm = ballot(hit);
  if (hm == 0ull) return;
  const uint32_t at = count + static_cast<uint32_t>(__popcll(hm & ((1ull << lane_id()) - 1ull)));
  if (hit && at < r.cap) {
    r.append_ids[region + at] = id;
    r.append_dists[region + at] = d;
  }
  count += static_cast<uint32_t>(__popcll(hm));
}

template <bool kIP, int kChunks>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(search_min_waves<kChunks, 0, 0>() ? search_min_waves<kChunks, 0, 0>() : 1, 8)))
    range_search_kernel(SearchParams p, FilterParams f, RangeParams r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kSpace = 0;
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x >> 6);
  const int W = static_cast<int>(blockDim.x >> 6);
  const Lds L = carve_lds<kSpace>(p, smem, wave);
  const uint64_t bit_words = (p.n + 31) / 32;
  const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * W + wave;
  uint32_t *slot_bits = p.overflow_bits + slot * bit_words;
  uint32_t *slot_dirty = p.dirty_words + slot * p.dirty_cap;
  constexpr bool kRegMerge = kChunks > 0 && kChunks <= 8;  // as the plain kernel's traversal merge
  const bool masked = f.allow != nullptr;                  // (uniform over the launch)

  for (;;) {
    uint32_t qi = 0;
    if (lane == 0) qi = atomicAdd(p.work_counter, 1u);
    qi = read_lane(qi, 0);
    if (qi >= p.nq) break;
    const uint32_t *mask =
        masked ? f.allow + static_cast<uint64_t>(f.mask_of_query != nullptr ? f.mask_of_query[qi] : 0u) * f.mask_words
               : nullptr;
    const float radius = r.radii[qi];
    const uint64_t region = static_cast<uint64_t>(qi) * r.cap;
    uint32_t count = 0;  // the query's hits so far (wave-uniform)
    Visited vs;
    PoolState ps;
    uint32_t n_dist = 0, n_expand = 0, n_dist_up = 0, n_hops_up = 0;
    query_begin<kIP, kChunks, kSpace>(p, L, qi, slot_bits, slot_dirty, nullptr, vs, ps, n_dist_up, n_hops_up,
                                      [&](bool has, uint32_t id, float d) {
                                        bool ok = has;
                                        if (has) {
                                          if (masked) ok = ((mask[id >> 5] >> (id & 31)) & 1u) != 0u;
                                          if (p.valid != nullptr) ok = ok && ((p.valid[id >> 5] >> (id & 31)) & 1u) != 0u;
                                        }
                                        range_offer(count, r, region, radius, ok, id, d);
                                      });

    // ---- best-first expansion: the plain searcher's loop ------------------------------------
    uint32_t pred = kEmpty, pred_v = kEmpty;  // adjacency prefetch of the predicted next pop
    while (ps.cur < ps.size) {
      const uint32_t u = pool_pop(ps, L);
      ++n_expand;
      uint32_t v = u == pred ? pred_v : adjacency_row(p, static_cast<int>(p.R), u);
      const int cnt = adjacency_count(static_cast<int>(p.R), v);
      bool act = lane < cnt;
      if (p.dedup_edges) {  // graphs with repeated ids in a row: keep the first occurrence only
        for (int j = 0; j < cnt; ++j) {
          const uint32_t vj = read_lane(v, j);
          if (j < lane && vj == v) act = false;
        }
      }
      if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin(vs);
      const bool fresh = visit(vs, v, act);
      const uint64_t fm = ballot(fresh);
      const int nf = __popcll(fm);
      pred = ps.cur < ps.size ? (L.pi[ps.cur] & kIdMask) : kEmpty;
      if (pred != kEmpty) pred_v = adjacency_row(p, static_cast<int>(p.R), pred, pred_v);
      if (nf == 0) continue;
      // compact fresh ids in adjacency order
      if (fresh) L.cid[__popcll(fm & ((1ull << lane) - 1ull))] = v;
      wave_sync();
      // each candidate's allow word (and validity word) goes out ahead of the row gather, as in the
      // filtered kernel
      const bool has = lane < nf;
      const uint32_t cid = has ? L.cid[lane] : 0u;
      uint32_t aw = 0xffffffffu, vw = 0xffffffffu;
      if (has) {
        if (masked) aw = mask[cid >> 5];
        if (p.valid != nullptr) vw = p.valid[cid >> 5];
      }
      space_distances<kIP, kChunks, kSpace>(p, L, L.cid, nf, L.cd);
      n_dist += nf;
      const float cd = has ? L.cd[lane] : 0.f;
      wave_sync();
      pool_merge<kRegMerge>(ps, L, has, cid, cd, [&](uint32_t nx) {
        if (nx != pred) {
          pred = nx;
          pred_v = adjacency_row(p, static_cast<int>(p.R), nx, pred_v);
        }
      });
      range_offer(count, r, region, radius, has && (((aw & vw) >> (cid & 31)) & 1u) != 0u, cid, cd);
    }

    query_end(p, L, ps, qi, n_dist, n_expand, n_dist_up, n_hops_up);  // p.k = 0: the four counters
    if (lane == 0) r.counts[qi] = count;
    visit_end(vs);
    wave_sync();
  }
}

// --------------------------------------------------------------------------------------------
// Range search, radius mode: range_search_kernel's traversal (phase 1, pop for pop), then a flood fill of
// the in-radius region it reached (phase 2).  Every (id, d) either phase measures whose row is valid and
// has d <= radius joins the query's frontier, in arrival order, whatever the allow mask says: the first
// m.cap of them are stored in the query's region of the global frontier buffer.  When the traversal pool
// has no unchecked entry left the stored frontier rows are expanded in that order: visit, distances,
// offers -- hits to the append list by phase 1's rule, in-radius rows to the frontier -- and nothing goes
// into the pool, so there is no merge.  The wave reads the frontier back 64 entries at a time, lane j
// taking entry cursor + j, with plain loads through the pointer it stored them by; the next row to
// expand is known exactly, so its adjacency row is issued before the distance pass.
// --------------------------------------------------------------------------------------------
// The in-radius rows among the lanes with `valid` join the frontier behind its `fcount` earlier ones, and
// the allowed ones among them the append list, as range_offer.  Without a mask the frontier's ballot is
// the hit ballot.
__device__ __forceinline__ void range_more_offer(uint32_t &count, uint32_t &fcount, const RangeParams &r,
                                                 const RangeMoreParams &m, uint64_t region, uint32_t *fr, float radius,
                                                 bool masked, bool valid, bool allowed, uint32_t id, float d) {
  const bool in = valid && d <= radius;
  const uint64_t im = ballot(in);
  if (im == 0ull) return;
  const uint64_t below = (1ull << lane_id()) - 1ull;
  const uint32_t fat = fcount + static_cast<uint32_t>(__popcll(im & below));
  if (in && fat < m.cap) fr[fat] = id;
  fcount += static_cast<uint32_t>(__popcll(im));
  bool hit = in;
  uint64_t hm = im;
  if (masked) {
    hit = in && allowed;
    hm = ballot(hit);
    if (hm == 0ull) return;
  }
  const uint32_t at = count + static_cast<uint32_t>(__popcll(hm & below));
  if (hit && at < r.cap) {
    r.append_ids[region + at] = id;
    r.append_dists[region + at] = d;
  }
  count += static_cast<uint32_t>(__popcll(hm));
}

template <bool kIP, int kChunks>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(search_min_waves<kChunks, 0, 0>() ? search_min_waves<kChunks, 0, 0>() : 1, 8)))
    range_more_search_kernel(SearchParams p, FilterParams f, RangeParams r, RangeMoreParams m) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kSpace = 0;
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x >> 6);
  const int W = static_cast<int>(blockDim.x >> 6);
  const Lds L = carve_lds<kSpace>(p, smem, wave);
  const uint64_t bit_words = (p.n + 31) / 32;
  const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * W + wave;
  uint32_t *slot_bits = p.overflow_bits + slot * bit_words;
  uint32_t *slot_dirty = p.dirty_words + slot * p.dirty_cap;
  constexpr bool kRegMerge = kChunks > 0 && kChunks <= 8;  // as the plain kernel's traversal merge
  const bool masked = f.allow != nullptr;                  // (uniform over the launch)
  const int R = static_cast<int>(p.R);

  for (;;) {
    uint32_t qi = 0;
    if (lane == 0) qi = atomicAdd(p.work_counter, 1u);
    qi = read_lane(qi, 0);
    if (qi >= p.nq) break;
    const uint32_t *mask =
        masked ? f.allow + static_cast<uint64_t>(f.mask_of_query != nullptr ? f.mask_of_query[qi] : 0u) * f.mask_words
               : nullptr;
    const float radius = r.radii[qi];
    const uint64_t region = static_cast<uint64_t>(qi) * r.cap;
    uint32_t *fr = m.frontier_ids + static_cast<uint64_t>(qi) * m.cap;
    uint32_t count = 0;   // the query's hits so far (wave-uniform)
    uint32_t fcount = 0;  // the rows that joined its frontier so far (wave-uniform)
    Visited vs;
    PoolState ps;
    uint32_t n_dist = 0, n_expand = 0, n_dist_up = 0, n_hops_up = 0;
    query_begin<kIP, kChunks, kSpace>(p, L, qi, slot_bits, slot_dirty, nullptr, vs, ps, n_dist_up, n_hops_up,
                                      [&](bool has, uint32_t id, float d) {
                                        bool valid = has, allowed = true;
                                        if (has) {
                                          if (masked) allowed = ((mask[id >> 5] >> (id & 31)) & 1u) != 0u;
                                          if (p.valid != nullptr) valid = ((p.valid[id >> 5] >> (id & 31)) & 1u) != 0u;
                                        }
                                        range_more_offer(count, fcount, r, m, region, fr, radius, masked, valid, allowed, id,
                                                         d);
                                      });

    // ---- phase 1: range_search_kernel's loop ---------------------------------------------------
    uint32_t pred = kEmpty, pred_v = kEmpty;  // adjacency prefetch of the predicted next pop
    while (ps.cur < ps.size) {
      const uint32_t u = pool_pop(ps, L);
      ++n_expand;
      uint32_t v = u == pred ? pred_v : adjacency_row(p, R, u);
      const int cnt = adjacency_count(R, v);
      bool act = lane < cnt;
      if (p.dedup_edges) {  // graphs with repeated ids in a row: keep the first occurrence only
        for (int j = 0; j < cnt; ++j) {
          const uint32_t vj = read_lane(v, j);
          if (j < lane && vj == v) act = false;
        }
      }
      if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin(vs);
      const bool fresh = visit(vs, v, act);
      const uint64_t fm = ballot(fresh);
      const int nf = __popcll(fm);
      pred = ps.cur < ps.size ? (L.pi[ps.cur] & kIdMask) : kEmpty;
      if (pred != kEmpty) pred_v = adjacency_row(p, R, pred, pred_v);
      if (nf == 0) continue;
      // compact fresh ids in adjacency order
      if (fresh) L.cid[__popcll(fm & ((1ull << lane) - 1ull))] = v;
      wave_sync();
      const bool has = lane < nf;
      const uint32_t cid = has ? L.cid[lane] : 0u;
      uint32_t aw = 0xffffffffu, vw = 0xffffffffu;
      if (has) {
        if (masked) aw = mask[cid >> 5];
        if (p.valid != nullptr) vw = p.valid[cid >> 5];
      }
      space_distances<kIP, kChunks, kSpace>(p, L, L.cid, nf, L.cd);
      n_dist += nf;
      const float cd = has ? L.cd[lane] : 0.f;
      wave_sync();
      pool_merge<kRegMerge>(ps, L, has, cid, cd, [&](uint32_t nx) {
        if (nx != pred) {
          pred = nx;
          pred_v = adjacency_row(p, R, nx, pred_v);
        }
      });
      range_more_offer(count, fcount, r, m, region, fr, radius, masked, has && ((vw >> (cid & 31)) & 1u) != 0u,
                       ((aw >> (cid & 31)) & 1u) != 0u, cid, cd);
    }
    query_end(p, L, ps, qi, n_dist, n_expand, n_dist_up, n_hops_up);  // p.k = 0: phase 1's four counters

    // ---- phase 2: the stored frontier rows, in arrival order -----------------------------------
    uint32_t cursor = 0, more = 0;
    for (;;) {
      const uint32_t stored = min(fcount, m.cap);
      if (cursor >= stored) break;
      // a window of the frontier: entries appended while it is walked lie past it
      const int wn = static_cast<int>(min(64u, stored - cursor));
      const uint32_t w = lane < wn ? fr[cursor + static_cast<uint32_t>(lane)] : kEmpty;
      uint32_t next_v = adjacency_row(p, R, read_lane(w, 0));
      for (int j = 0; j < wn; ++j) {
        const uint32_t v = next_v;
        const int cnt = adjacency_count(R, v);
        bool act = lane < cnt;
        if (p.dedup_edges) {
          for (int e = 0; e < cnt; ++e) {
            const uint32_t ve = read_lane(v, e);
            if (e < lane && ve == v) act = false;
          }
        }
        if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin(vs);
        const bool fresh = visit(vs, v, act);
        const uint64_t fm = ballot(fresh);
        const int nf = __popcll(fm);
        // the window's next row, ahead of the distance pass
        if (j + 1 < wn) next_v = adjacency_row(p, R, read_lane(w, j + 1), next_v);
        if (nf == 0) continue;
        if (fresh) L.cid[__popcll(fm & ((1ull << lane) - 1ull))] = v;
        wave_sync();
        const bool has = lane < nf;
        const uint32_t cid = has ? L.cid[lane] : 0u;
        uint32_t aw = 0xffffffffu, vw = 0xffffffffu;
        if (has) {
          if (masked) aw = mask[cid >> 5];
          if (p.valid != nullptr) vw = p.valid[cid >> 5];
        }
        space_distances<kIP, kChunks, kSpace>(p, L, L.cid, nf, L.cd);
        more += nf;
        const float cd = has ? L.cd[lane] : 0.f;
        wave_sync();
        range_more_offer(count, fcount, r, m, region, fr, radius, masked, has && ((vw >> (cid & 31)) & 1u) != 0u,
                         ((aw >> (cid & 31)) & 1u) != 0u, cid, cd);
      }
      cursor += static_cast<uint32_t>(wn);
    }

    if (lane == 0) {
      r.counts[qi] = count;
      if (m.more != nullptr) {
        m.more[static_cast<uint64_t>(qi) * 2] = fcount;
        m.more[static_cast<uint64_t>(qi) * 2 + 1] = more;
      }
    }
    visit_end(vs);
    wave_sync();
  }
}

__device__ __forceinline__ uint32_t range_pow2(uint32_t n) {
  uint32_t p2 = 1;
  while (p2 < n) p2 <<= 1;
  return p2;
}

// One workgroup per query: the query's min(count, cap) stored rows into LDS, padded to a power of two
// with (FLT_MAX, kEmpty), a bitonic sort on (distance, id) under float comparison -- the float itself is
// the key, so -0.0 ties with +0.0, the id decides, and the measured bits come back out -- then the
// sorted rows and the empty tail to the outputs.  Hits are never NaN (d <= radius held), and a pad sorts
// behind every hit: no row has id kEmpty.
__global__ void __launch_bounds__(256) range_sort_kernel(RangeParams r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *sd = reinterpret_cast<float *>(smem);
  uint32_t *si = reinterpret_cast<uint32_t *>(smem) + range_pow2(r.cap);
  const uint64_t region = static_cast<uint64_t>(blockIdx.x) * r.cap;
  const uint32_t n = min(r.counts[blockIdx.x], r.cap);
  const uint32_t n2 = range_pow2(n);  // <= range_pow2(r.cap): the launch's LDS
  for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) {
    sd[i] = i < n ? r.append_dists[region + i] : FLT_MAX;
    si[i] = i < n ? r.append_ids[region + i] : kEmpty;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= n2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) {
        const uint32_t o = i ^ j;
        if (o > i) {
          const float da = sd[i], db = sd[o];
          const uint32_t ia = si[i], ib = si[o];
          const bool b_first = db < da || (db == da && ib < ia);
          const bool a_first = da < db || (da == db && ia < ib);
          if ((i & k) == 0u ? b_first : a_first) {
            sd[i] = db;
            sd[o] = da;
            si[i] = ib;
            si[o] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = threadIdx.x; i < r.cap; i += blockDim.x) {
    r.out_ids[region + i] = i < n ? si[i] : kEmpty;
    r.out_dists[region + i] = i < n ? sd[i] : FLT_MAX;
  }
}

// --------------------------------------------------------------------------------------------
// Range search of SQ8 codes: filtered_sq8_search_kernel's traversal, pop for pop -- the query encoded to
// codes, code-to-code distances without a validity test, the spill levels and their prefetch -- with the
// candidate pool replaced by range_search_kernel's append list, cut at the query's code radius
// (r.radii[i]).  Every (id, code distance) the traversal hands to pool.insert, in that order, whose row is
// valid, allowed by the query's mask (f.allow == nullptr: no mask) and has d_code <= the code radius is a
// candidate: r.counts[i] counts them all, the first r.cap are stored in arrival order.
// range_rerank_kernel then measures the stored ones exactly.  No LDS beyond the plain SQ8 searcher's
// (carve_lds is unchanged, p.k = 0: query_end writes the counters only).
// --------------------------------------------------------------------------------------------

// range_offer under candidate_offer's discipline: the validity bitmap is read last, and only when some allowed
// lane is within the code radius, so no validity word is live across the distance pass.
__device__ __forceinline__ void range_sq8_offer(const SearchParams &p, uint32_t &count, const RangeParams &r, uint64_t region,
                                                float radius, bool allowed, uint32_t id, float d) {
  bool ok = allowed && d <= radius;
  if (ballot(ok) == 0ull) return;
  if (p.valid != nullptr && ok) ok = ((p.valid[id >> 5] >> (id & 31)) & 1u) != 0u;
  range_offer(count, r, region, radius, ok, id, d);
}

template <bool kIP, int kChunks, int kSpace>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(search_min_waves<kChunks, kSpace, 0>() ? search_min_waves<kChunks, kSpace, 0>() : 1, 8)))
    range_sq8_search_kernel(SearchParams p, FilterParams f, RangeParams r) {
  static_assert(space_sq8<kSpace>(), "SQ8 codes");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool kTab = space_tab<kSpace>();
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x >> 6);
  const int W = static_cast<int>(blockDim.x >> 6);
  const Lds L = carve_lds<kSpace>(p, smem, wave);
  fill_shared<kSpace>(p, L);  // the workgroup's only barrier: every wave passes it, with or without a query
  const uint64_t bit_words = (p.n + 31) / 32;
  const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * W + wave;
  uint32_t *slot_bits = p.overflow_bits + slot * bit_words;
  uint32_t *slot_dirty = p.dirty_words + slot * p.dirty_cap;
  uint16_t *slot_stab = (kTab && p.spill_table) ? p.spill_table + (slot << p.stab_log2) : nullptr;
  const bool masked = f.allow != nullptr;  // (uniform over the launch)

  for (;;) {
    uint32_t qi = 0;
    if (lane == 0) qi = atomicAdd(p.work_counter, 1u);
    qi = read_lane(qi, 0);
    if (qi >= p.nq) break;
    const uint32_t *mask =
        masked ? f.allow + static_cast<uint64_t>(f.mask_of_query != nullptr ? f.mask_of_query[qi] : 0u) * f.mask_words
               : nullptr;
    // the query's state across the loop, all wave-uniform: the code radius, the region base, the count
    const float radius = r.radii[qi];
    const uint64_t region = static_cast<uint64_t>(qi) * r.cap;
    uint32_t count = 0;
    Visited vs;
    PoolState ps;
    uint32_t n_dist = 0, n_expand = 0, n_dist_up = 0, n_hops_up = 0;
    query_begin<kIP, kChunks, kSpace>(p, L, qi, slot_bits, slot_dirty, slot_stab, vs, ps, n_dist_up, n_hops_up,
                                      [&](bool has, uint32_t id, float d) {
                                        bool allowed = has;
                                        if (has && masked) allowed = ((mask[id >> 5] >> (id & 31)) & 1u) != 0u;
                                        range_sq8_offer(p, count, r, region, radius, allowed, id, d);
                                      });

    // ---- best-first expansion: the plain SQ8 searcher's loop ----------------------------------
    uint32_t pred = kEmpty, pred_v = kEmpty;  // adjacency prefetch of the predicted next pop
    uint32_t pre_u = kEmpty;                  // second-level state read one expansion ahead (spill_prefetch)
    uint64_t pre_lo = 0ull, pre_hi = 0ull;
    while (ps.cur < ps.size) {
      const uint32_t u = pool_pop(ps, L);
      ++n_expand;
      uint32_t v = u == pred ? pred_v : adjacency_row(p, static_cast<int>(p.R), u);
      const int cnt = adjacency_count(static_cast<int>(p.R), v);
      bool act = lane < cnt;
      if (p.dedup_edges) {  // graphs with repeated ids in a row: keep the first occurrence only
        for (int j = 0; j < cnt; ++j) {
          const uint32_t vj = read_lane(v, j);
          if (j < lane && vj == v) act = false;
        }
      }
      if (!vs.spilled && vs.count + 64 > vs.limit) spill_begin<kTab>(vs);
      const bool fresh = visit<kTab>(vs, v, act, u == pre_u, pre_lo, pre_hi);
      // the pred_v load below issues after this visit's spill-table stores and bitset atomics: the
      // second-level prefetch's wait for pred_v is its wait for them (as in hnsw_search_kernel)
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" ::: "memory");
      pre_u = kEmpty;  // consumed: the prefetched state describes the table only up to this visit's stores
      pre_lo = pre_hi = 0ull;
      const uint64_t fm = ballot(fresh);
      const int nf = __popcll(fm);
      pred = ps.cur < ps.size ? (L.pi[ps.cur] & kIdMask) : kEmpty;
      if (pred != kEmpty) pred_v = adjacency_row(p, static_cast<int>(p.R), pred, pred_v);
      if (nf == 0) continue;
      // compact fresh ids in adjacency order
      if (fresh) L.cid[__popcll(fm & ((1ull << lane) - 1ull))] = v;
      wave_sync();
      // each candidate's allow word goes out ahead of the code rows, by the lane that will hold the
      // candidate at the merge; it is used only after the distances, so its latency is the rows'
      const bool has = lane < nf;
      uint32_t aw = 0xffffffffu;
      if (has && masked) aw = mask[L.cid[lane] >> 5];
      space_distances<kIP, kChunks, kSpace>(p, L, L.cid, nf, L.cd, [&]() {
        // the predicted next expansion's second-level state, behind this expansion's first row pass
        if (vs.spilled && pred != kEmpty && !(p.spill_flags & 1u)) {
          spill_prefetch(vs, pred_v, lane < static_cast<int>(p.R), pre_lo, pre_hi);
          pre_u = pred;
        }
      });
      n_dist += nf;
      const uint32_t cid = has ? L.cid[lane] : 0u;
      const float cd = has ? L.cd[lane] : 0.f;
      wave_sync();
      pool_merge(ps, L, has, cid, cd, [&](uint32_t nx) {
        if (nx != pred) {
          pred = nx;
          pred_v = adjacency_row(p, static_cast<int>(p.R), nx, pred_v);
        }
      });
      range_sq8_offer(p, count, r, region, radius, has && ((aw >> (cid & 31)) & 1u) != 0u, cid, cd);
    }

    query_end(p, L, ps, qi, n_dist, n_expand, n_dist_up, n_hops_up);  // p.k = 0: the four counters
    if (lane == 0) r.counts[qi] = count;
    visit_end(vs);
    wave_sync();
  }
}

// The rerank of the range search of SQ8 codes.  One wave per (query, block of 64 stored candidates): a block
// past the query's min(r.counts[i], r.cap) stored candidates ends at once, so a query with few candidates costs
// one short block and a small batch with long lists still fills the CUs.  The wave stages the rerank query
// (p.queries) in LDS once, measures its candidates on their f32 rows eight at a time -- row_distance_kernel's
// passes: the arithmetic of rerank_kernel -- and writes the exact distance over the code distance in the append
// list.  A candidate with d_exact > r.radii[i] (the exact radius here; NaN compares false) becomes the sort's pad
// (FLT_MAX, kEmpty); the survivors are added to hits[i], zeroed before the launch: one popcount of a ballot and
// one atomic per wave.  range_sort_kernel then runs as it is, with r.counts the candidate counts: the pads sort
// behind every hit and come out as the empty tail.
template <bool kIP>
__global__ void __launch_bounds__(64) range_rerank_kernel(SearchParams p, RangeParams r, uint32_t *hits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *q = reinterpret_cast<float *>(smem);
  uint32_t *lid = reinterpret_cast<uint32_t *>(smem + static_cast<size_t>(p.stride) * 4);
  float *ld = reinterpret_cast<float *>(lid + 64);
  const int lane = lane_id();
  const uint64_t qi = blockIdx.x;
  const uint32_t n = min(r.counts[qi], r.cap);
  const uint32_t b = blockIdx.y * 64u;
  if (b >= n) return;  // (uniform over the wave)
  const uint32_t cnt = min(64u, n - b);
  const uint64_t at = qi * r.cap + b + static_cast<uint32_t>(lane);
  const bool has = static_cast<uint32_t>(lane) < cnt;
  if (has) lid[lane] = r.append_ids[at];
  const float *qsrc = p.queries + qi * p.q_stride;
  for (uint32_t e = lane; e < p.stride; e += 64) q[e] = e < p.dim ? qsrc[e] : 0.f;
  wave_sync();
  for (uint32_t c = 0; c < cnt; c += 8) row_distances<kIP, 0>(p, q, lid + c, static_cast<int>(min(8u, cnt - c)), ld + c);
  const float d = has ? ld[lane] : 0.f;
  const bool hit = has && d <= r.radii[qi];
  if (has) {
    r.append_dists[at] = hit ? d : FLT_MAX;
    if (!hit) r.append_ids[at] = kEmpty;
  }
  const uint64_t hm = ballot(hit);
  if (lane == 0 && hm != 0ull) atomicAdd(hits + qi, static_cast<uint32_t>(__popcll(hm)));
}
}  // namespace

// The range kernels: the filtered kernels' set.
template <int... kChunks>
static const void *range_symbol_of(int chunks, bool ip) {
  const void *sym = nullptr;
  ((chunks == kChunks ? (sym = ip ? reinterpret_cast<const void *>(&range_search_kernel<true, kChunks>)
                                  : reinterpret_cast<const void *>(&range_search_kernel<false, kChunks>),
                         0)
                      : 0),
   ...);
  return sym;
}

static const void *range_kernel_symbol(uint32_t dim, bool generic, bool ip) {
  const void *sym = range_symbol_of<4, 8, 16, 24, 30, 32>(search_chunks(dim, generic), ip);
  return sym != nullptr ? sym : range_symbol_of<0>(0, ip);
}

hipError_t launch_range_search(const SearchParams &p, const FilterParams &f, const RangeParams &r, int grid, int waves,
                               size_t lds, hipStream_t stream) {
  SearchParams arg = p;
  FilterParams farg = f;
  RangeParams rarg = r;
  void *args[] = {&arg, &farg, &rarg};
  return hipLaunchKernel(range_kernel_symbol(p.dim, p.generic, p.ip), dim3(grid), dim3(64 * waves), args, lds, stream);
}

hipError_t range_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, range_kernel_symbol(dim, generic, ip), 64 * waves, lds);
}

// The radius-mode range kernels: the same set.
template <int... kChunks>
static const void *range_more_symbol_of(int chunks, bool ip) {
  const void *sym = nullptr;
  ((chunks == kChunks ? (sym = ip ? reinterpret_cast<const void *>(&range_more_search_kernel<true, kChunks>)
                                  : reinterpret_cast<const void *>(&range_more_search_kernel<false, kChunks>),
                         0)
                      : 0),
   ...);
  return sym;
}

static const void *range_more_kernel_symbol(uint32_t dim, bool generic, bool ip) {
  const void *sym = range_more_symbol_of<4, 8, 16, 24, 30, 32>(search_chunks(dim, generic), ip);
  return sym != nullptr ? sym : range_more_symbol_of<0>(0, ip);
}

hipError_t launch_range_more_search(const SearchParams &p, const FilterParams &f, const RangeParams &r,
                                    const RangeMoreParams &m, int grid, int waves, size_t lds, hipStream_t stream) {
  SearchParams arg = p;
  FilterParams farg = f;
  RangeParams rarg = r;
  RangeMoreParams marg = m;
  void *args[] = {&arg, &farg, &rarg, &marg};
  return hipLaunchKernel(range_more_kernel_symbol(p.dim, p.generic, p.ip), dim3(grid), dim3(64 * waves), args, lds, stream);
}

hipError_t range_more_search_occupancy(uint32_t dim, bool generic, bool ip, int waves, size_t lds, int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, range_more_kernel_symbol(dim, generic, ip), 64 * waves,
                                                      lds);
}

hipError_t launch_range_sort(const RangeParams &r, uint64_t nq, hipStream_t stream) {
  if (nq == 0) return hipSuccess;
  uint32_t p2 = 1;
  while (p2 < r.cap) p2 <<= 1;
  hipLaunchKernelGGL(range_sort_kernel, dim3(static_cast<uint32_t>(nq)), dim3(256), static_cast<size_t>(p2) * 8, stream, r);
  return hipGetLastError();
}

// The range kernels of SQ8 codes: the filtered SQ8 kernels' set.
template <int kSpace, int... kChunks>
static const void *range_sq8_symbol_of(int chunks, bool ip) {
  const void *sym = nullptr;
  ((chunks == kChunks ? (sym = ip ? reinterpret_cast<const void *>(&range_sq8_search_kernel<true, kChunks, kSpace>)
                                  : reinterpret_cast<const void *>(&range_sq8_search_kernel<false, kChunks, kSpace>),
                         0)
                      : 0),
   ...);
  return sym;
}

static const void *range_sq8_kernel_symbol(uint32_t dim, int sq8_order, bool ip) {
  const int chunks = search_chunks(dim, false);
  const void *sym = sq8_order == 2 ? range_sq8_symbol_of<2, 4, 24, 30>(chunks, ip)
                                   : range_sq8_symbol_of<1, 4, 24, 30>(chunks, ip);
  if (sym != nullptr) return sym;
  return sq8_order == 2 ? range_sq8_symbol_of<2, 0>(0, ip) : range_sq8_symbol_of<1, 0>(0, ip);
}

hipError_t launch_range_sq8_search(const SearchParams &p, const FilterParams &f, const RangeParams &r, int grid, int waves,
                                   size_t lds, hipStream_t stream) {
  SearchParams arg = p;
  FilterParams farg = f;
  RangeParams rarg = r;
  void *args[] = {&arg, &farg, &rarg};
  return hipLaunchKernel(range_sq8_kernel_symbol(p.dim, p.sq8_order, p.ip), dim3(grid), dim3(64 * waves), args, lds,
                         stream);
}

hipError_t range_sq8_search_occupancy(uint32_t dim, int sq8_order, bool ip, int waves, size_t lds, int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, range_sq8_kernel_symbol(dim, sq8_order, ip), 64 * waves,
                                                      lds);
}

hipError_t launch_range_rerank(const SearchParams &p, const RangeParams &r, uint32_t *hits, hipStream_t stream) {
  if (p.nq == 0) return hipSuccess;
  const size_t lds = static_cast<size_t>(p.stride) * 4 + 128 * 4;
  const dim3 grid(static_cast<uint32_t>(p.nq), (r.cap + 63) / 64);
  if (p.ip) {
    hipLaunchKernelGGL(range_rerank_kernel<true>, grid, dim3(64), lds, stream, p, r, hits);
  } else {
    hipLaunchKernelGGL(range_rerank_kernel<false>, grid, dim3(64), lds, stream, p, r, hits);
  }
  return hipGetLastError();
}

}  // namespace alaya_amd
