/*
 * alaya_hip.h -- C ABI of the MI355X search engine (libalaya_hip.so).
 *
 * This is the drop-in boundary for AlayaLite's search hot path.  Plain pointers and sizes only;
 * every call returns an int status (ALAYA_OK == 0) and alaya_last_error() gives the message of
 * the last failure on the calling thread.  Host buffers are copied; *_device variants take device
 * pointers and a hipStream_t (passed as void*) and are asynchronous on that stream.
 *
 * Streams: an index keeps per-index scratch (work counter, visited-set spill area, flat and SQ8
 * candidate buffers).  Every launching call orders itself after the previous launching call on the
 * index (a hipStreamWaitEvent when the streams differ), so calls on different streams serialise on
 * the device instead of racing; calls that replace device buffers (set_base, set_graph, set_sq8,
 * build_graph, reserve, enable_updates, destroy) first wait for those launches to finish.  Calls on
 * one index from several host threads are serialised by the index's lock.
 *
 * Reference interfaces each group replaces (paths relative to the AlayaLite repo root):
 *   alaya_index_*            PyIndex<HNSWBuilder<RawSpace>, Space> state and lifetime
 *                            (python/include/index.hpp:85-506, PyIndexInterface :508-587)
 *   alaya_index_set_base     RawSpace ctor/fit + SequentialStorage (include/space/raw_space.hpp:81-140,
 *                            include/storage/sequential_storage.hpp:53-84) -- rows moved to HBM
 *   alaya_index_set_graph    Graph + OverlayGraph (include/index/graph/graph.hpp:44-158,
 *                            overlay_graph.hpp:26-144) -- adjacency moved to HBM
 *   alaya_index_batch_search PyIndex::batch_search / batch_search_with_distance
 *                            (python/include/index.hpp:289-451) -> GraphSearchJob::search
 *                            (include/executor/jobs/graph_search_job.hpp:221-299) on the device
 *   alaya_index_search       PyIndex::search (index.hpp:236-258) -> search_solo (:302-371)
 *   alaya_index_distances    RawSpace::QueryComputer::operator() (raw_space.hpp:297-304) over
 *                            simd::l2_sqr / ip_sqr (include/simd/distance_l2.ipp:729-742,
 *                            distance_ip.ipp:739-751) -- the metric plugin surface
 *                            (include/space/space_concepts.hpp:31-73)
 *   alaya_graph_*            HNSWBuilder::build_graph (include/index/graph/hnsw/hnsw_builder.hpp:98-194)
 *                            and Graph::save/load (graph.hpp:165-238)
 */
#ifndef ALAYA_HIP_H_
#define ALAYA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALAYA_OK 0
#define ALAYA_ERR_ARG 1      /* invalid argument (Python: ValueError)            */
#define ALAYA_ERR_RUNTIME 2  /* runtime failure (Python: RuntimeError)           */
#define ALAYA_ERR_DEVICE 3   /* HIP error / no device (Python: RuntimeError)     */

/* MetricType values of include/utils/metric_type.hpp */
#define ALAYA_METRIC_L2 0
#define ALAYA_METRIC_IP 1
#define ALAYA_METRIC_COS 2
/* OR-ed into the metric of alaya_index_set_base / alaya_graph_build_hnsw: the rows are a non-float
 * DataType (int8, uint8, int32, uint32, double) cast to float, and distances follow the generic
 * branch of l2_sqr<T> / ip_sqr<T> (include/simd/distance_l2.ipp:735-741, distance_ip.ipp:744-750:
 * one float accumulator over the elements in order) instead of the AVX2 float kernel. */
#define ALAYA_DIST_GENERIC 0x100

typedef struct alaya_index alaya_index;
typedef struct alaya_graph alaya_graph;

const char *alaya_last_error(void);
/* Build provenance (no reference counterpart): "source=<16 hex digits of sha256 over the library's
 * sources and headers> arch=gfx950 hipcc=<compiler> built=<UTC time>", fixed when the library was
 * compiled (alayalite_amd/_build.py).  bench.py and smoke() compare the source hash with the tree. */
const char *alaya_build_info(void);
/* Number of visible HIP devices (0 when none). */
int alaya_device_count(int *count);
/* Roofline calibration (no reference counterpart): the best of `iters` streaming reads of a
 * `bytes`-byte device buffer (>= 1 MiB) over three load shapes and two occupancies, in GB/s -- the
 * measured bandwidth ceiling bench.py reports beside the 8 TB/s HBM3E figure. */
int alaya_hbm_stream_read(int device, uint64_t bytes, int iters, double *gbs);
/* A HIP stream whose launches may use every CU of `device` but `reserved_cus` (spread over the CU
 * numbering), so kernels of other streams -- the shard exchange's RCCL all_gather -- find free CUs
 * while a persistent search runs; searches launched on it size their grid to the CUs left.  No
 * reference counterpart (the reference is single-process CPU code). */
int alaya_stream_create_reserving(int device, uint32_t reserved_cus, void **stream);
int alaya_stream_destroy(void *stream);

/* ---- host graph (builder + reference on-disk format) --------------------------------------- */
/* data: n x dim float32 row-major (normalised already for COS).  seed 100 = reference default. */
int alaya_graph_build_hnsw(const float *data, uint64_t n, uint32_t dim, int metric, uint32_t R,
                           uint32_t ef_construction, uint32_t num_threads, uint64_t seed,
                           alaya_graph **out);
int alaya_graph_load(const char *path, int id_bytes, alaya_graph **out);
/* valid_bitmap (nullable): the graph storage bitmap, ceil(n/8) bytes; a node removed with
 * GraphUpdateJob::remove has its bit cleared in the reference's file (sequential_storage.hpp:94-100). */
int alaya_graph_save(const alaya_graph *g, const char *path, int id_bytes, uint64_t capacity,
                     const uint8_t *valid_bitmap);
/* sizes: n, R, has_overlay, upper_R, ep, max_level, n_upper_edges, n_eps */
int alaya_graph_info(const alaya_graph *g, uint64_t *n, uint32_t *R, int *has_overlay,
                     uint32_t *upper_R, uint32_t *ep, uint32_t *max_level,
                     uint64_t *n_upper_edges, uint32_t *n_eps);
/* copy out: l0[n*R], levels[n], upper_off[n], upper_edges[n_upper_edges], eps[n_eps]; any NULL skipped */
int alaya_graph_export(const alaya_graph *g, uint32_t *l0, uint32_t *levels, uint64_t *upper_off,
                       uint32_t *upper_edges, uint32_t *eps);
/* build a graph object from host arrays (levels == NULL -> NSG-style eps) */
int alaya_graph_import(uint64_t n, uint32_t R, const uint32_t *l0, const uint32_t *levels,
                       const uint64_t *upper_off, const uint32_t *upper_edges,
                       uint64_t n_upper_edges, uint32_t upper_R, uint32_t ep, const uint32_t *eps,
                       uint32_t n_eps, alaya_graph **out);
void alaya_graph_free(alaya_graph *g);

/* ---- device index ---------------------------------------------------------------------------- */
int alaya_index_create(int device, alaya_index **out);
void alaya_index_destroy(alaya_index *ix);
/* rows: n x dim float32 host array (row pitch dim).  valid_bitmap: ceil(n/8) bytes in the
 * SequentialStorage layout (bit i%8 of byte i/8 set = valid) or NULL for all valid. */
int alaya_index_set_base(alaya_index *ix, const float *rows, uint64_t n, uint32_t dim, int metric,
                         const uint8_t *valid_bitmap);
int alaya_index_set_graph(alaya_index *ix, const alaya_graph *g);
/* Batched search on host buffers.  ids: nq x k; dists (nullable): nq x k; counters (nullable):
 * nq x 4 uint32 = (n_dist, n_expand, n_dist_upper, n_hops_upper). */
int alaya_index_batch_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                             uint32_t ef, uint32_t *ids, float *dists, uint32_t *counters);
/* Same on device buffers, asynchronous on `stream` (hipStream_t; NULL = default stream). */
int alaya_index_batch_search_device(alaya_index *ix, const float *d_queries, uint64_t nq,
                                    uint32_t k, uint32_t ef, uint32_t *d_ids, float *d_dists,
                                    uint32_t *d_counters, void *stream);
/* The per-shard search of a base-range sharded index (no reference counterpart): as
 * alaya_index_batch_search_device, except that result slots past the pool (shard rows < k, or
 * ef < k) hold (0xffffffff, FLT_MAX) instead of the reference's (0, 0.0), so they sort after every
 * real candidate in the cross-shard merge.  d_dists is required. */
int alaya_index_shard_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k,
                                    uint32_t ef, uint32_t *d_ids, float *d_dists, uint32_t *d_counters,
                                    void *stream);
/* Filtered graph search: the k nearest rows among those a per-query mask allows (f32 rows; an index
 * with SQ8 codes is refused here and served by alaya_index_filtered_search_sq8 below).  The traversal is alaya_index_batch_search's at the same ef -- the same
 * overlay descent, pool of capacity ef, visited set and pops, so the four counters are the same --
 * and beside it a second pool of capacity k, the result pool, is offered every (id, distance) the
 * traversal hands to its own pool, in that order, whose row is valid and allowed.  ids / dists hold
 * the result pool in order, then empty slots (0xffffffff, FLT_MAX).  A candidate the traversal pool
 * rejects can still enter the result pool, and k may exceed ef; 1 <= k <= 224, ef >= 1.
 * allow_words: n_masks x ceil(n / 32) uint32 words, bit i % 32 of word i / 32 of a mask = row i (the
 * validity bitmap's layout as 32-bit words); n = the index's row count, removed rows included; bits
 * past n are ignored.  mask_of_query: nq indices below n_masks, the mask of each query; may be NULL
 * when n_masks == 1.  Environment ALAYA_FILTER_GRID=n (diagnostics, read per launch) holds the launch
 * to n workgroups, so every wave runs several queries one after the other; results never depend on it. */
int alaya_index_filtered_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k, uint32_t ef,
                                const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                uint32_t *ids, float *dists, uint32_t *counters);
/* Same on device buffers, asynchronous on `stream`; the indices of d_mask_of_query are not checked. */
int alaya_index_filtered_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k, uint32_t ef,
                                       const uint32_t *d_allow_words, uint32_t n_masks,
                                       const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists,
                                       uint32_t *d_counters, void *stream);
/* Through search: filtered graph search that expands through disallowed neighbours (f32 rows; opt-in, the
 * default stays alaya_index_filtered_search).  A neighbour the query may not see is not measured and not kept:
 * the search steps through it to its own neighbours, so the pool of ef entries holds allowed rows only and ef
 * keeps its usual meaning.  It is meant for small and middling allowed shares, where the plain traversal loses
 * recall, and the caller chooses: at the same ef it computes about 5x the plain traversal's distances at a share
 * of 0.5 and fewer from 0.05 down, and it reads one adjacency row per row stepped through, which is what its time
 * goes to at small shares ("Round 17", has the measured sweep; below a share of about 0.1
 * alaya_index_flat_search_filtered is exact and faster).
 *
 * passable(v): the query's allow bit of row v is set and, on an index with a validity bitmap, v is valid.
 * For one query, with a traversal pool `pool` (LinearPool, capacity ef), a result pool `result` (capacity k)
 * and a visited set:
 *   1. Entry.  The overlay descent is alaya_index_batch_search's, with distances on any row; n_dist_upper and
 *      n_hops_upper are unchanged.  The level-0 entry is marked visited and inserted into `pool` whatever its
 *      bit; it is offered to `result` only when passable.  On a graph without overlay this holds for every
 *      entry point in turn, repeats included.
 *   2. Pop and direct pass.  While pool.has_next(): u = pool.pop(), n_expand += 1.  Walk u's level-0 row in
 *      adjacency order, to the first empty slot (graphs flagged for repeated edges: first occurrence only).
 *      Each neighbour v not yet visited is marked visited.  If passable(v): d = dist(q, v), n_dist += 1,
 *      pool.insert(v, d), result.insert(v, d).  Otherwise v is appended to this pop's through list T; no
 *      distance is computed for it and it never enters a pool.
 *   3. Through pass.  For each w in T, in order: n_through += 1, then walk w's level-0 row under the same
 *      rules.  A row x that is not passable is skipped and is not marked visited (it may later be stepped
 *      through as somebody's direct neighbour).  A passable x not yet visited is marked visited, then
 *      d = dist(q, x), n_dist += 1, pool.insert(x, d), result.insert(x, d).  One level only: no recursion.
 *   4. Output.  `result` in order, then empty slots (0xffffffff, FLT_MAX).  counters per query are (n_dist,
 *      n_expand, n_dist_upper, n_hops_upper), nq x 4 as everywhere; n_through (nullable) receives nq uint32.
 * The kernel gathers candidates of several through rows into one distance pass and one merge; the observable
 * state equals that of the sequential inserts in the arrival order above.  So: with a mask of all ones and no
 * bitmap T is always empty, and the answer and the four counters are alaya_index_filtered_search's (hence
 * alaya_index_batch_search's); a removed row is stepped through instead of entering the pool at FLT_MAX; with
 * an all-zero mask the query ends after the entry's pop with n_dist = 0 and every slot empty.
 * Arguments, their errors and ALAYA_FILTER_GRID as for alaya_index_filtered_search; an index with SQ8 codes is
 * refused. */
int alaya_index_filtered_search_hop(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k, uint32_t ef,
                                    const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                    uint32_t *ids, float *dists, uint32_t *counters, uint32_t *n_through);
/* Same on device buffers, asynchronous on `stream`; the indices of d_mask_of_query are not checked. */
int alaya_index_filtered_search_hop_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k, uint32_t ef,
                                           const uint32_t *d_allow_words, uint32_t n_masks,
                                           const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists,
                                           uint32_t *d_counters, uint32_t *d_n_through, void *stream);
/* Filtered graph search of an index with SQ8 codes (alaya_index_set_sq8): the k nearest rows, by exact
 * f32 distance, among the candidates a filtered SQ8 traversal collects.
 *   1. Traversal: alaya_index_batch_search_sq8's at the same ef -- the query encoded to codes, code-to-code
 *      distances (no validity test in the distance: removed rows are traversed like any other), the same
 *      overlay descent, pool of capacity ef, visited set and pops; the four counters are those of
 *      alaya_index_batch_search_sq8(..., rerank = 0).
 *   2. Candidate pool: a second pool of capacity m = `pool`, k <= m <= 224, is offered every (id, code
 *      distance) the traversal hands to its own pool, in that order, whose row is valid and allowed.
 *      pool = 0 means min(224, max(k, ef)): the whole traversal pool, under the cap.
 *   3. Rerank: the candidates are rescored with the f32 distance of rerank_queries (NULL = queries) to their
 *      f32 rows; ids / dists hold the first k under (exact distance, id), equal pairs in pool order, then
 *      empty slots (0xffffffff, FLT_MAX).  No id-0 entries and no zero fill (this is not
 *      alaya_index_batch_search_sq8's reference rerank); a candidate the traversal met twice stays twice.
 * A larger m costs candidate-pool merges in the search stage and m row reads in the rerank, and buys
 * candidates whose code distance misorders them against the k-th exact one.  allow_words, n_masks,
 * mask_of_query and ALAYA_FILTER_GRID as for alaya_index_filtered_search.  For the COS metric the callers of
 * the Index layer pass the un-normalised queries to the traversal and the normalised ones to the rerank, as
 * for alaya_index_batch_search_sq8.  An index without SQ8 codes, k or pool outside 1..224, pool < k, ef = 0
 * and a shape whose LDS does not fit are argument errors.  Environment ALAYA_FILTER_RERANK=0 (diagnostics, read
 * per launch) runs the search stage alone, to time it: ids and dists are then left unwritten. */
int alaya_index_filtered_search_sq8(alaya_index *ix, const float *queries, const float *rerank_queries, uint64_t nq,
                                    uint32_t k, uint32_t ef, uint32_t pool, const uint32_t *allow_words,
                                    uint32_t n_masks, const uint32_t *mask_of_query, uint32_t *ids, float *dists,
                                    uint32_t *counters);
/* Same on device buffers, asynchronous on `stream`; the indices of d_mask_of_query are not checked. */
int alaya_index_filtered_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries,
                                           uint64_t nq, uint32_t k, uint32_t ef, uint32_t pool,
                                           const uint32_t *d_allow_words, uint32_t n_masks,
                                           const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists,
                                           uint32_t *d_counters, void *stream);
/* Range search: every row the graph traversal measures within a radius of the query (f32 rows; an index with
 * SQ8 codes is refused).  For query i with radius r_i = radii[i] and cap C = max_results, 1 <= C <= 4096:
 *   1. Traversal: alaya_index_batch_search's at the same ef -- the same overlay descent, pool of capacity ef,
 *      visited set and pops -- so the four counters are equal, as for alaya_index_filtered_search.  The radius
 *      does not steer it: it neither stops early nor expands past what ef gives.
 *   2. Hits: the subsequence, in arrival order, of the (id, d) the traversal hands to its pool (the entry offers
 *      included) whose row is valid, is allowed by the query's mask when masks are given, and has d <= r_i as
 *      an f32 comparison (inclusive).  A removed row never qualifies, whatever the radius.  d is the index's
 *      distance: squared L2, or -(q.b) for IP and COS (a radius of -0.8 on normalised rows = cosine >= 0.8).
 *   3. counts[i] = the number of hits, not capped.
 *   4. The first min(counts[i], C) hits to arrive are stored and returned in row i of ids / dists (nq x C),
 *      ordered by (distance, id) under float comparison -- -0.0 ties with +0.0 and the id decides -- with the
 *      measured distance bits; the remaining slots hold (0xffffffff, FLT_MAX).
 *   5. counts[i] > C means the list is truncated: the stored rows are the first C to arrive, NOT the C nearest.
 *      A caller that needs them all raises max_results or lowers the radius.
 *   6. A graph without overlay whose entry-point list repeats an id offers it twice, and it stays twice.
 * allow_words / n_masks / mask_of_query as for alaya_index_filtered_search; allow_words == NULL with
 * n_masks == 0 (and mask_of_query == NULL) means no mask.  counters (nullable): nq x 4.  max_results outside
 * 1..4096, ef == 0, a NaN radius (host entry only) and a mask shape the filtered entries refuse are argument
 * errors.  ALAYA_FILTER_GRID as for alaya_index_filtered_search.  Environment ALAYA_RANGE_SORT=0 (diagnostics,
 * read per launch) runs the search stage alone, to time it: ids and dists are then left unwritten. */
int alaya_index_range_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t ef, const float *radii,
                             uint32_t max_results, const uint32_t *allow_words, uint32_t n_masks,
                             const uint32_t *mask_of_query, uint32_t *counts, uint32_t *ids, float *dists,
                             uint32_t *counters);
/* Same on device buffers, asynchronous on `stream`: it never waits on the stream, so d_radii (nq floats) is not
 * read here and a NaN radius simply matches nothing; the indices of d_mask_of_query are not checked.  The
 * append list between the two kernels is the index's own scratch. */
int alaya_index_range_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t ef,
                                    const float *d_radii, uint32_t max_results, const uint32_t *d_allow_words,
                                    uint32_t n_masks, const uint32_t *d_mask_of_query, uint32_t *d_counts,
                                    uint32_t *d_ids, float *d_dists, uint32_t *d_counters, void *stream);
/* Range search, radius mode: the range search above, which then keeps expanding while rows within the radius
 * turn up -- a flood fill of the in-radius region the traversal reached.  ef says where the fill starts.  For
 * query i with radius r_i, result cap C = max_results (1..4096) and frontier cap F = max_frontier (1..16384):
 *   1. Phase 1 is alaya_index_range_search, unchanged: alaya_index_batch_search's traversal at ef on the f32
 *      rows, the same pops, the same four counters, the same hit rule (valid, allowed when masks are given,
 *      d <= r_i as an f32 comparison, arrival order).
 *   2. The frontier: every (id, d) that phase 1 or phase 2 computes, entry offers included, joins the query's
 *      frontier in arrival order when its row is valid and d <= r_i.  The allow mask does not matter here: a
 *      disallowed in-radius row is not a hit but is continued through.  frontier[i] counts the rows that
 *      joined and is not capped; the first F to arrive are stored.  A removed row never joins; a repeated
 *      entry point joins twice and stays twice.
 *   3. Phase 2: when the traversal pool has no unchecked entry left, the stored frontier rows are expanded in
 *      arrival order, whether or not phase 1 had already popped them.  For each, the level-0 row is read
 *      (repeated ids dropped as in phase 1); neighbours not yet visited are marked visited, measured in
 *      adjacency order and offered: hits follow rule 1, the frontier rule 2.  Nothing is inserted into the
 *      traversal pool.  Phase 2 ends when the cursor reaches the end of the stored frontier, so it expands
 *      min(frontier[i], F) rows; more_dist[i] counts the distances it computed.
 *   4. counts, the stored min(counts, C) first hits and their order by (distance, id) are rules 3-6 of
 *      alaya_index_range_search, applied to the hit stream of both phases.  The four counters stay phase 1's,
 *      so they still equal alaya_index_batch_search's.
 *   5. frontier[i] > F means the continuation was cut: in-radius rows past the first F were counted and
 *      returned as hits, but not expanded.
 *   6. (An implementation may skip the adjacency read of a frontier row it can prove phase 1 expanded: such a
 *      row yields no fresh neighbour, so hits, frontier and more_dist are the same either way.  This one reads
 *      every row.)
 * With no truncation (counts <= C, frontier <= F), no mask and no removed rows the returned set contains phase
 * 1's hits and is closed: every level-0 neighbour of a returned row that lies within the radius is returned too.
 * With a radius below every measured distance phase 2 does nothing.  A radius that takes in most of the index
 * makes phase 2 read up to F adjacency rows and measure up to F x R rows per query.
 * more (nullable): nq x 2, (frontier[i], more_dist[i]).  The arguments, refusals and environment switches are
 * alaya_index_range_search's; max_frontier outside 1..16384 is an argument error as well. */
int alaya_index_range_search_radius(alaya_index *ix, const float *queries, uint64_t nq, uint32_t ef, const float *radii,
                                    uint32_t max_results, const uint32_t *allow_words, uint32_t n_masks,
                                    const uint32_t *mask_of_query, uint32_t *counts, uint32_t *ids, float *dists,
                                    uint32_t *counters, uint32_t max_frontier, uint32_t *more);
/* Same on device buffers, asynchronous on `stream`, as alaya_index_range_search_device; the frontier (nq x
 * max_frontier ids) is the index's own scratch beside the append list. */
int alaya_index_range_search_radius_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t ef,
                                           const float *d_radii, uint32_t max_results, const uint32_t *d_allow_words,
                                           uint32_t n_masks, const uint32_t *d_mask_of_query, uint32_t *d_counts,
                                           uint32_t *d_ids, float *d_dists, uint32_t *d_counters, void *stream,
                                           uint32_t max_frontier, uint32_t *d_more);
/* Range search of an index with SQ8 codes: the traversal runs on the codes, the stored candidates are measured
 * exactly.  For query i with radius r_i = radii[i], code radius c_i = code_radii[i] and cap C = max_results,
 * 1 <= C <= 4096:
 *   1. Traversal: alaya_index_batch_search_sq8's at the same ef -- the query encoded to codes, code-to-code
 *      distances with no validity test, the same overlay descent, pool of ef entries, visited levels and pops --
 *      so the four counters are equal, as for alaya_index_filtered_search_sq8.  Neither radius steers it.
 *   2. Candidates: the subsequence, in arrival order, of the (id, d_code) the traversal hands to its pool (the
 *      entry offers included) whose row is valid, is allowed by the query's mask when masks are given, and has
 *      d_code <= c_i as an f32 comparison (inclusive).  cand[i] = their number, not capped; the first
 *      min(cand[i], C) are stored.
 *   3. Rerank: every stored candidate is measured exactly -- the raw-space f32 distance of the rerank query
 *      (rerank_queries, NULL = queries) to the row's f32 row, the arithmetic of alaya_index_batch_search_sq8's
 *      rerank.  A stored candidate with d_exact <= r_i (inclusive f32 comparison) is a hit; counts[i] = the number
 *      of hits, so counts[i] <= min(cand[i], C).
 *   4. Row i of ids / dists (nq x C) holds the hits by (exact distance, id) under float comparison, with the
 *      exact distance bits; the remaining slots hold (0xffffffff, FLT_MAX).
 *   5. cand[i] > C means the list is truncated: candidates past the first C to arrive were never reranked.  The
 *      reranked ones are the first C to arrive, NOT the C nearest, as for alaya_index_range_search.
 *   6. A repeated entry point is a candidate twice, and stays twice.
 *   7. Code and exact distances disagree in both directions, so c_i is the caller's: c_i above r_i admits rows
 *      whose code distance overstates the exact one (the rerank cut removes the rest); c_i = +inf makes every
 *      valid, allowed measured row a candidate.  COS: the Index layer passes the query as given to the
 *      traversal and the normalised one to the rerank, as for alaya_index_filtered_search_sq8.
 * Masks, counters and ALAYA_FILTER_GRID as for alaya_index_range_search.  An index without SQ8 codes, max_results
 * outside 1..4096, ef == 0, a NaN in radii or code_radii (host entry only), a mask shape the filtered entries
 * refuse and a shape whose LDS does not fit are argument errors.  Environment ALAYA_RANGE_SORT=0 (diagnostics,
 * read per launch) runs the search stage alone, to time it: cand and counters are written, counts are zero, ids
 * and dists are left unwritten; ALAYA_RANGE_SORT=2 runs the search and the rerank without the sort: counts are
 * written too.  alaya_index_range_search[_radius][_device] go on refusing an SQ8 index. */
int alaya_index_range_search_sq8(alaya_index *ix, const float *queries, const float *rerank_queries, uint64_t nq,
                                 uint32_t ef, const float *radii, const float *code_radii, uint32_t max_results,
                                 const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                 uint32_t *counts, uint32_t *cand, uint32_t *ids, float *dists, uint32_t *counters);
/* Same on device buffers, asynchronous on `stream`: it never waits on the stream, so neither radius array is
 * read here and a NaN simply matches nothing; the indices of d_mask_of_query are not checked.  d_counts is zeroed
 * on the stream before the rerank adds to it; the append list is the index's own scratch. */
int alaya_index_range_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries,
                                        uint64_t nq, uint32_t ef, const float *d_radii, const float *d_code_radii,
                                        uint32_t max_results, const uint32_t *d_allow_words, uint32_t n_masks,
                                        const uint32_t *d_mask_of_query, uint32_t *d_counts, uint32_t *d_cand,
                                        uint32_t *d_ids, float *d_dists, uint32_t *d_counters, void *stream);
/* ---- device graph construction (Index.fit on the MI355X) ------------------------------------
 * Replaces HNSWBuilder::build_graph (include/index/graph/hnsw/hnsw_builder.hpp:98-194) over hnswlib
 * add_point (include/index/graph/hnsw/hnswlib.hpp:652-751), from the index's own rows
 * (alaya_index_set_base; COS rows already normalised).  M = R/2, M0 = R, ef = max(ef_construction,
 * M), levels drawn exactly as the reference draws them from `seed` (100 in the reference).  Points
 * are inserted in label order in batches of max(1, min(max_batch, inserted / batch_div)) (0 ->
 * defaults 16 / 65536); within a batch every point runs searchBaseLayer + the neighbour heuristic
 * on the device against the graph as it stood before the batch, then reverse edges are merged per
 * destination (append, or prune with the heuristic).  `refine` extra level-0 passes per batch let
 * the batch's points re-select among each other once they are linked in (2 recommended; with
 * batch_div = max_batch = 1 and refine = 0 the insertion is sequential, as the reference's).  The result is installed as the index's
 * search graph and a host copy is returned in *out (nullable).  stats (nullable, 8 x u64):
 * batches, kernel launches, list prunes, appended edges, heuristic distances, device time (us),
 * largest batch, max level. */
int alaya_index_build_graph(alaya_index *ix, uint32_t R, uint32_t ef_construction, uint64_t seed,
                            uint32_t batch_div, uint32_t max_batch, uint32_t refine, alaya_graph **out,
                            uint64_t *stats);
/* ---- bulk growth (Index.add) ----------------------------------------------------------------
 * Appends `count` rows (ix->dim floats each, COS rows already normalised) to an index that has rows
 * and an installed HNSW graph over them -- device-built, host-built, loaded, or changed by
 * alaya_index_insert / alaya_index_remove -- by continuing the batched build above: the graph is the
 * state after rows [0, n0), the new rows are inserted in label order, their levels are the tail of
 * the draw for n0 + count rows from `seed`, the batch sizes follow from the rows inserted so far and
 * the first batch starts from the graph's own entry point and max level.  So when n0 is a batch
 * boundary of the schedule for all rows, build(n0 rows) + extend(the rest) is build(all rows) bit
 * for bit (alaya_build_batches lists the boundaries).  Needs an overlay whose lists are R wide, R
 * even in 2..64 and n0 + count < 2^31; anything else is ALAYA_ERR_ARG and leaves the index as it was.
 * Every per-row device buffer grows once per call, so one large call beats many small ones.
 *
 * Removed rows (cleared validity bits): the build's searches measure them as a query does (FLT_MAX)
 * and the neighbour selection drops them, so no new row links to a removed row on any level, no
 * removed row receives an edge and the removed rows' own lists stay as they are.  Rows the update
 * job rewrote may repeat ids; they are taken as they are.
 * SQ8 indexes: the new rows' codes are encoded on the device with the quantizer the index was given
 * (alaya_index_set_sq8's min / max, alaya_sq8_encode's arithmetic).  The quantizer is not retrained:
 * a value outside the fitted range of its dimension clamps to code 0 or 255.  alaya_index_read_sq8
 * copies codes of rows [first, first + count) back (dim bytes per row).
 * The new rows are valid, the grown graph stays installed, a host copy of the whole graph is
 * returned in *out (nullable), and an update mirror (alaya_index_enable_updates), if there is one,
 * follows with its record of removals kept.  stats as alaya_index_build_graph's, for this call's
 * batches alone. */
int alaya_index_extend_graph(alaya_index *ix, const float *rows, uint64_t count, uint32_t ef_construction,
                             uint64_t seed, uint32_t batch_div, uint32_t max_batch, uint32_t refine,
                             alaya_graph **out, uint64_t *stats);
int alaya_index_read_sq8(alaya_index *ix, uint64_t first, uint64_t count, uint8_t *codes);
/* Host only: the batch ends of the schedule of rows [start, n) with the given levels, for a graph
 * over rows [0, start) whose entry point is `ep` (a build from scratch: start = 1, ep = 0).  ends
 * NULL: count only.  Every end is a row count at which alaya_index_extend_graph continues the
 * schedule exactly. */
int alaya_build_batches(const uint32_t *levels, uint64_t n, uint64_t start, uint32_t ep, uint32_t batch_div,
                        uint32_t max_batch, uint64_t *ends, uint64_t *n_batches);
/* ---- online updates (Index.insert / Index.remove) ------------------------------------------
 * Device-mirror primitives, for a host that keeps its own graph and update job (the reference's
 * GraphUpdateJob, include/executor/jobs/graph_update_job.hpp:49-137) and patches HBM after each
 * change:  reserve capacity (rows, validity, adjacency; contents kept), write rows at [first,
 * first+count), overwrite level-0 adjacency rows, set or clear a validity bit
 * (SequentialStorage::insert/remove, sequential_storage.hpp:77-100). */
int alaya_index_reserve(alaya_index *ix, uint64_t capacity);
int alaya_index_write_rows(alaya_index *ix, uint64_t first, const float *rows, uint64_t count);
int alaya_index_write_edges(alaya_index *ix, const uint32_t *ids, const uint32_t *edges, uint64_t count);
int alaya_index_set_valid(alaya_index *ix, uint64_t id, int valid);
/* Or let the engine run the update job: enable_updates copies the graph, rows and bitmap into a
 * host mirror (capacity = the index capacity, IndexParams.capacity_).  insert = PyIndex::insert ->
 * insert_and_update (graph_update_job.hpp:65-89): search_solo for R neighbours at ef on the device,
 * append the node, update() every node that gained an edge, patch HBM.  search_query is the query
 * as search_solo sees it and row the vector as RawSpace::insert stores it (they differ only for COS,
 * which normalises at both steps).  new_id = UINT64_MAX when the index is full.  remove =
 * GraphUpdateJob::remove (:91-103): record the node's edges, clear its validity bit.  export_*
 * return the mirror (for save). */
int alaya_index_enable_updates(alaya_index *ix, const alaya_graph *g, const float *rows, uint64_t n,
                               uint64_t capacity, const uint8_t *valid_bitmap);
int alaya_index_insert(alaya_index *ix, const float *search_query, const float *row, uint32_t ef,
                       uint64_t *new_id);
int alaya_index_remove(alaya_index *ix, uint64_t id);
int alaya_index_export_graph(alaya_index *ix, alaya_graph **out);
/* rows: n x dim (nullable), valid_bitmap: (n+7)/8 bytes (nullable); *n = stored rows. */
int alaya_index_export_rows(alaya_index *ix, float *rows, uint8_t *valid_bitmap, uint64_t *n);
/* out[q*n + i] = metric distance(queries[q], row ids[i]), bit-exact with the search kernel. */
int alaya_index_distances(alaya_index *ix, const float *queries, uint64_t nq, const uint32_t *ids,
                          uint32_t n, float *out);
/* Diagnostic build of the search kernel: also returns per-query s_memtime cycles per phase,
 * stamps[nq*8] = (init+descent, pop, adjacency+visited, distances, merge, expansions after the
 * visited table spilled, whole query, adjacency-prefetch hits).  space 0 = f32 rows (same ids as
 * alaya_index_batch_search), 1 = the SQ8 codes (no rerank; d = 768 is stamped, others run plain). */
int alaya_index_profile_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                               uint32_t ef, int space, uint32_t *ids, uint32_t *counters, uint64_t *stamps);
/* ---- SQ8 search space (SQ8Space: include/space/sq8_space.hpp, quant/sq8.hpp) --------------------
 * Per-dimension min/max (SQ8Quantizer::fit, sq8.hpp:99-113) and codes (quantize, :118-130). */
int alaya_sq8_train(const float *data, uint64_t n, uint32_t dim, float *min_v, float *max_v);
int alaya_sq8_encode(const float *data, uint64_t n, uint32_t dim, const float *min_v,
                     const float *max_v, uint8_t *codes, uint32_t num_threads);
/* Attach SQ8 codes (n x dim) to an index whose f32 rows are set.  order: the reduction order of
 * the reference kernel the host would pick -- 2 = l2/ip_sqr_sq8_avx512 (AVX-512F hosts),
 * 1 = the AVX2 variants (distance_l2.ipp:694-708, distance_ip.ipp:703-716). */
int alaya_index_set_sq8(alaya_index *ix, const uint8_t *codes, uint64_t n, uint32_t dim,
                        const float *min_v, const float *max_v, int order);
/* PyIndex::batch_search with SearchSpace = SQ8Space (index.hpp:289-346): graph search on the SQ8
 * codes (queries encoded in-kernel), then a rerank on the f32 rows with rerank_queries (NULL =
 * queries).  rerank: 0 = none (the SQ8 ids and distances), 1 = PyIndex::rerank as the reference
 * runs it, including its ef-k zero entries (index.hpp:450-488), 2 = corrected: the whole ef pool
 * is rescored (no id-0 duplicates); result slots beyond the candidates hold (0, 0.0). */
int alaya_index_batch_search_sq8(alaya_index *ix, const float *queries, const float *rerank_queries,
                                 uint64_t nq, uint32_t k, uint32_t ef, int rerank, uint32_t *ids,
                                 float *dists, uint32_t *counters);
/* Same on device buffers, asynchronous on `stream`; d_rerank_queries NULL = d_queries. */
int alaya_index_batch_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries,
                                        uint64_t nq, uint32_t k, uint32_t ef, int rerank, uint32_t *d_ids,
                                        float *d_dists, uint32_t *d_counters, void *stream);
/* The per-shard search of a base-range sharded SQ8 index (no reference
 * counterpart): the SQ8 graph search plus PyIndex::rerank (index.hpp:337-345, 450-488) on this
 * shard's rows.  The reference's id-0 quirk (the ef - k zero-filled res_pool slots, :301, rescored
 * as row 0) belongs to global row 0 only: with holds_row0 != 0 (the shard whose local row 0 is
 * global row 0) the rerank is exactly alaya_index_batch_search_sq8_device's rerank = 1; otherwise
 * only the k search ids are rescored.  Result slots without a candidate hold (0xffffffff, FLT_MAX),
 * so they sort after every real candidate in the cross-shard merge.  With one shard the merged
 * result equals the reference's batch_search.  d_dists is required. */
int alaya_index_shard_search_sq8_device(alaya_index *ix, const float *d_queries, const float *d_rerank_queries,
                                        uint64_t nq, uint32_t k, uint32_t ef, int holds_row0, uint32_t *d_ids,
                                        float *d_dists, uint32_t *d_counters, void *stream);
/* ---- flat (exhaustive) exact k-NN, L2 / IP / COS, any dim, 1 <= k <= 224 ------------------------
 * No reference implementation (IndexType::FLAT is enum-only, include/index/index_type.hpp:28); the
 * analogue is find_exact_gt (include/utils/evaluate.hpp:29-62).  An MFMA pass ranks every row
 * by |b|^2 - 2 q.b (L2) or by -2 q.b (IP, and COS: as for the graph search the caller has normalised
 * the rows and the queries; ALAYA_DIST_GENERIC bases are refused) and keeps a shortlist -- q.b from a single-pass f16 contraction on power-of-two
 * scaled operands (rows of <= 224 floats) or a bf16 hi/lo split (3 bf16 MFMAs; wider rows), each
 * error bounded and folded into the proof below (alaya_index_flat_last_contraction; environment
 * ALAYA_FLAT_CONTRACTION selects one, ALAYA_FLAT_F32=1 the f32 MFMA form); rows wider than 224
 * floats are scanned in K slabs.  The single-pass scan reads f16 tile records of the rows that the
 * index builds at its first flat search and keeps (K/16 KB + 256 B per 32 rows: 264.5 MB for
 * 1M x 128), rebuilding them after any change to the rows, their count or the validity bitmap;
 * a prescan over a sample of them seeds every query's threshold.  The shortlist (32 per row chunk,
 * folded into a 128/256-entry list for k > 24) is rescored with the exact device metric
 * (l2_sqr_avx2 / ip_sqr_avx2 order; IP distances are -(q.b)) and sorted by (distance, id).  A query
 * whose shortlist cannot be proven to hold the exact top-k (error bound in flat_kernels.hip for L2,
 * flat_bound.h for inner products) is flagged; the host API recomputes it
 * exhaustively and reports how many it did.  The device variant is asynchronous on `stream` and
 * only writes d_flags[q] = 1 for such a query (its d_ids row is then not proven exact): the caller
 * recomputes it, e.g. through alaya_index_flat_search. */
int alaya_index_flat_search(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                            uint32_t *ids, float *dists, uint32_t *n_recomputed);
int alaya_index_flat_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k,
                                   uint32_t *d_ids, float *d_dists, uint32_t *d_flags, void *stream);
/* The contraction the last flat search ranked its shortlist with (introspection): 2 = single-pass f16
 * (the default for rows of <= 224 floats: one f16 MFMA per 16 k on operands scaled by powers of two,
 * error bound ~2^-10 |q||b|; the host API reruns a launch with the split if more than 1 % of its
 * queries are flagged), 1 = bf16 hi/lo split (3 bf16 MFMAs; wide rows and out-of-range scales),
 * 0 = f32 MFMA; -1 before any flat search.  Environment ALAYA_FLAT_CONTRACTION = f16 | bf16x3 | f32
 * selects one. */
int alaya_index_flat_last_contraction(const alaya_index *ix, int *contraction);
/* ---- exact filtered k-NN: a scan over the allowed rows, for small allowed shares -----------------
 * Stands in for find_exact_gt (include/utils/evaluate.hpp:29-62) over a subset: query i's answer is the
 * rows that are valid and that its mask allows, ordered by (distance, id), the first k of them; the
 * remaining slots hold (0xffffffff, FLT_MAX), alaya_index_flat_search's convention.  The distance is
 * the index's metric in f32 in the reference's order from the start (l2_sqr_avx2; ip_sqr_avx2 for IP
 * and COS, -(q.b), the caller having normalised rows and queries for COS) -- the bits of
 * alaya_index_flat_search's and alaya_index_distances' results -- so nothing is flagged or recomputed.
 * No graph is needed; an index with SQ8 codes is scanned on its f32 rows; ALAYA_DIST_GENERIC bases are
 * refused.  Rows or queries with non-finite distances are not covered.
 * allow_words, n_masks, mask_of_query: as for alaya_index_filtered_search (n_masks x ceil(n / 32) words,
 * bit i % 32 of word i / 32 of a mask = row i, bits past n ignored whatever they hold; mask_of_query may
 * be NULL with one mask), and so are the argument checks: 1 <= k <= 224, n_masks >= 1.
 * Masks are served one after another: (mask AND validity) is compacted into an ascending id list, the
 * mask's queries are scanned against ranges of that list with each gathered row reused across a tile
 * of queries, and the per-range lists are merged.  The work grows with allowed rows x queries: above a
 * share of a few per cent the graph search or the unmasked flat search is faster.  Environment
 * ALAYA_FLAT_FILTER_CHUNK_ROWS=r (diagnostics, read per call) forces the id-list entries per range;
 * results never depend on it. */
int alaya_index_flat_search_filtered(alaya_index *ix, const float *queries, uint64_t nq, uint32_t k,
                                     const uint32_t *allow_words, uint32_t n_masks, const uint32_t *mask_of_query,
                                     uint32_t *ids, float *dists);
/* Same (find_exact_gt, evaluate.hpp:29-62, over a subset) on device buffers, the mask words on the device,
 * launched on `stream`.  The call waits on `stream` for each mask's allowed-row count (the scan's grid
 * depends on it) and, with more than one mask, reads d_mask_of_query back and checks it; when it
 * returns, the last mask's launches may still be running.  d_dists may be NULL. */
int alaya_index_flat_search_filtered_device(alaya_index *ix, const float *d_queries, uint64_t nq, uint32_t k,
                                            const uint32_t *d_allow_words, uint32_t n_masks,
                                            const uint32_t *d_mask_of_query, uint32_t *d_ids, float *d_dists,
                                            void *stream);
/* Introspection of the last call above (find_exact_gt over a subset has no counterpart): out[0] = allowed
 * valid rows summed over the masks that had queries, out[1] = row chunks of the last scan, out[2] = its
 * query tile, out[3] = scan launches. */
int alaya_index_flat_filtered_last(const alaya_index *ix, uint64_t *out);
/* The scan's launch plan as pure host arithmetic (no device; find_exact_gt over a subset has no
 * counterpart): for n_allowed rows, nq queries of one mask, k, rows of `stride` floats and `cus` compute
 * units, out[0] = rows per chunk (a multiple of the 32 rows a wave takes per pass; ALAYA_FLAT_FILTER_CHUNK_ROWS
 * rounded up to one, unless a single query tile's lists would then pass the cap), out[1] = chunks
 * (out[0] out[1] >= n_allowed, and no more than fill the CUs twice over at this tile), out[2] = queries per
 * workgroup (4, 8 or 16), out[3] = queries per scan launch (a multiple of out[2]; the launches cover nq),
 * out[4] = bytes of partial lists of one launch, at most 256 MiB for any nq.  ALAYA_ERR_ARG if k is
 * outside 1..224 or the rows are too wide for the LDS. */
int alaya_flat_filtered_plan(uint64_t n_allowed, uint64_t nq, uint32_t k, uint32_t stride, uint32_t cus,
                             uint64_t *out);
/* ---- exact range search: every eligible row within a radius, by a scan of the rows ---------------
 * The exact counterpart of alaya_index_range_search (no reference counterpart: find_exact_gt,
 * include/utils/evaluate.hpp:29-62, keeps the k nearest).  For query i with radius r_i = radii[i] and cap
 * C = max_results, 1 <= C <= 4096:
 * 1. Eligible rows: every row below the index's row count that is valid (the validity bitmap) and, when masks
 *    are given, allowed by the query's mask.  allow_words, n_masks, mask_of_query: alaya_index_filtered_search's
 *    format (bits past n ignored); allow_words == NULL with n_masks == 0 means no mask, as for
 *    alaya_index_range_search.  No graph is needed; an index with SQ8 codes is scanned on its f32 rows;
 *    ALAYA_DIST_GENERIC bases are refused.
 * 2. Distance: the index's metric in f32 in the reference's order from the start (l2_sqr_avx2; ip_sqr_avx2
 *    negated for IP and COS) -- the bits of alaya_index_flat_search_filtered and alaya_index_distances.  No
 *    approximate contraction, no bound, no flag, no recompute.
 * 3. Hits: a row is a hit when d <= r_i as an f32 comparison, inclusive.  A radius of -inf matches nothing;
 *    +inf and FLT_MAX match every eligible row with a finite distance.  A NaN radius is ALAYA_ERR_ARG on the
 *    host entry; on the device entry it matches nothing, and the device entry never waits on the stream to
 *    read radii.
 * 4. counts[i] (uint32) is the exact number of hits, never capped.
 * 5. Row i of ids / dists (nq x C) holds min(counts[i], C) hits ordered by (distance, id) under float
 *    comparison (-0.0 ties with +0.0, the id decides), with the distance bits of rule 2; the remaining slots
 *    hold (0xffffffff, FLT_MAX).  counts[i] > C means the list is truncated: it then holds the C hits with the
 *    smallest ids, because the scan meets rows in ascending id -- alaya_index_range_search's "first C to
 *    arrive, not the C nearest", with a fixed arrival order.
 * 6. The result is a function of the inputs alone: not of the row chunking, the grid, the query tile, or how
 *    a batch is split over launches.  Each (row chunk, query) pair has its own hit list and count, written by
 *    one wave in id order, and the lists are concatenated in chunk order.
 * 7. No workgroup waits for another.
 * Masks are served one after another: (mask AND validity) is compacted into an ascending id list (no mask:
 * the validity bitmap, or all-ones words), the mask's queries are scanned against chunks of that list, a
 * gather joins the chunk lists and range_sort_kernel orders each row.  The work grows with eligible rows x
 * queries; this is the f32 scan of alaya_index_flat_search_filtered, not the MFMA scan of
 * alaya_index_flat_search.  Environment (diagnostics, read per call; results never depend on them):
 * ALAYA_FLAT_RANGE_CHUNK_ROWS=r forces the id-list entries per chunk, ALAYA_FLAT_RANGE_STAGING_BYTES=b the
 * cap on one scan launch's staging (default 256 MiB; raised to what one query tile of one chunk needs),
 * ALAYA_FLAT_RANGE_STAGES=1 | 2 stops after the scans | the gathers, to time them (outputs then incomplete). */
int alaya_index_flat_range_search(alaya_index *ix, const float *queries, uint64_t nq, const float *radii,
                                  uint32_t max_results, const uint32_t *allow_words, uint32_t n_masks,
                                  const uint32_t *mask_of_query, uint32_t *counts, uint32_t *ids, float *dists);
/* Same on device buffers, launched on `stream`.  The call waits on `stream` for each mask's eligible-row count
 * (the scan's grid depends on it) and, with more than one mask, reads d_mask_of_query back and checks it; when
 * it returns, the last launches may still be running.  Every slot of d_counts, d_ids and d_dists is written. */
int alaya_index_flat_range_search_device(alaya_index *ix, const float *d_queries, uint64_t nq, const float *d_radii,
                                         uint32_t max_results, const uint32_t *d_allow_words, uint32_t n_masks,
                                         const uint32_t *d_mask_of_query, uint32_t *d_counts, uint32_t *d_ids,
                                         float *d_dists, void *stream);
/* Introspection of the last call above: of the last mask that had queries, out[0] = eligible rows, out[1] = row
 * chunks, out[2] = query tile, out[3] = scan launches; over all masks, out[4] = eligible rows summed,
 * out[5] = scan launches. */
int alaya_index_flat_range_last(const alaya_index *ix, uint64_t *out);
/* The range scan's launch plan as pure host arithmetic (no device): for n_eligible rows, nq queries of one
 * mask, the cap, rows of `stride` floats and `cus` compute units, out[0] = rows per chunk (a multiple of 32;
 * ALAYA_FLAT_RANGE_CHUNK_ROWS rounded up to one, unless a single query tile's staging would then pass the
 * cap), out[1] = chunks (no more than fill the CUs twice over at this tile), out[2] = queries per workgroup
 * (4, 8 or 16), out[3] = queries per scan launch (a multiple of out[2]), out[4] = stored hits per (chunk,
 * query) = min(max_results, out[0]), out[5] = staging bytes of one launch = out[1] x min(nq, out[3]) x
 * (8 out[4] + 4), within the staging cap for any nq.  ALAYA_ERR_ARG if max_results is outside 1..4096 or the
 * rows are too wide for the LDS. */
int alaya_flat_range_plan(uint64_t n_eligible, uint64_t nq, uint32_t max_results, uint32_t stride, uint32_t cus,
                          uint64_t *out);
/* Tuning / introspection: LDS visited-table size (log2 slots, 6..16; 0 = automatic) and layout
 * (0 = automatic, 1 = compact 16-bit slots, 2 = 32-bit id slots, 3 = compact with probe distance
 * capped at 2, a test hook for the spill-on-long-probe path).  Results never depend on either:
 * the visited set is exact (DynamicBitset, include/utils/query_utils.hpp:69-115). */
int alaya_index_set_hash_log2(alaya_index *ix, uint32_t log2_slots);
int alaya_index_set_visited_mode(alaya_index *ix, int mode);
/* Distance helpers (-1 automatic, 0 off, 1 on; environment ALAYA_HELPERS overrides): a searcher
 * whose batch has no query left computes the distances of a sibling searcher's predicted next
 * expansion (same workgroup) into an LDS memo the sibling reads.  Replaces nothing in the reference:
 * its coroutine scheduler keeps every worker busy to the end of a batch
 * (include/executor/worker.hpp:47,111-136); results never depend on it (the searcher still does
 * every visit, merge and pop; memo distances are the same function of the same inputs).
 * alaya_index_help_stats: of the last search with helpers, how many of its fresh distances
 * (the n_dist counters) the searchers took from a memo, in how many expansions every fresh distance
 * came from it, and how many rows the helpers computed (waits for that search; 0 without helpers). */
int alaya_index_set_helpers(alaya_index *ix, int mode);
int alaya_index_help_stats(alaya_index *ix, uint64_t *memo_dists, uint64_t *memo_expansions,
                           uint64_t *helper_rows);
/* Candidate screen of the wide-row f32 L2 graph search (d = 512 / 768 / 960 / 1024): once a query's
 * pool is full, the fresh candidates of an expansion are first measured on a low-precision copy of
 * their rows, and only those whose proven lower bound on the exact distance is below the pool's worst
 * distance read their f32 row.  Two copies exist, each built at the first search that uses it and
 * freed with the base: the rows as f16 (n x stride x 2 bytes + 4 bytes per row), and 8-bit records
 * (per row a 16-byte header {e_row, lo, scale, 0} and stride codes for lo + code x scale, padded to
 * a multiple of 64 bytes: 1024 bytes at d = 960; the first 8 bytes of the padding hold sum code and
 * sum code^2 as u32).  Environment ALAYA_SEARCH_SCREEN, read per launch:
 * 0 = no screen, 1 = the f16 copy, 8 = the 8-bit records in f32 arithmetic, 9 = the same records
 * against the query's own 8-bit codes (integer dot products), unset = the default of the width.
 * Results and counters never depend on it.  alaya_index_screen_stats: of the last graph search,
 * how many candidates were screened and how many of those were screened out (waits for that search;
 * 0, 0 when it did not screen). */
int alaya_index_screen_stats(alaya_index *ix, uint64_t *screened, uint64_t *screened_out);
/* The screen's bound, evaluated on the host by the function the kernel calls (screen_bound.h):
 * out[i] <= the reference's f32 L2 distance of any q, x of `dim` elements for which d_tilde[i] is an
 * f32 sum in any order of (q_j - y_j)^2 over a copy y of x, and e_row[i] >= ||x - y||_2. */
int alaya_screen_lower_bound(const float *d_tilde, const float *e_row, uint64_t n, uint32_t dim, float *out);
/* The 8-bit screening copy of n rows of dim elements, made on the host by the functions the device
 * uses (screen_bound.h): codes (n x dim), header (n x 4: e_row, lo, scale, 0) and values (n x dim: the
 * f32 value each code stands for).  e_row >= ||row - values||_2, +inf for a row that is not finite. */
int alaya_screen_u8_quantize(const float *rows, uint64_t n, uint32_t dim, uint8_t *codes, float *header,
                             float *values);
/* The integer screen's bound (ALAYA_SEARCH_SCREEN=9) for the n pairs (queries[i], rows[i]) of dim <= 4096
 * elements, made on the host by the functions the kernel calls (screen_bound.h).  Both vectors go
 * through the 8-bit quantiser above; with q^, y^ the real-valued grids lo + code x scale of the two,
 * d_in[i] <= ||q^ - y^||^2 (0 = no bound), e_sum[i] >= ||x - y^|| + ||q - q^||, bound[i] <= the
 * reference's f32 L2 distance of the pair, and sums (n x 5) holds the exact integers the kernel works
 * from: sum a, sum a^2 (query codes), sum c, sum c^2 (row codes: the two u32 a record carries after
 * its codes), sum a c. */
int alaya_screen_int_bound(const float *queries, const float *rows, uint64_t n, uint32_t dim, float *d_in,
                           float *e_sum, float *bound, uint32_t *sums);
/* The flat search's inner-product bound, evaluated on the host by the functions the merge kernels
 * call (flat_bound.h).  alaya_flat_ip_slack: out[i] >= |d_ref + C~| for the reference's f32 distance
 * d_ref = -(q.b) (ip_sqr_avx2) and the scan's contraction C~ (0 = f32 MFMA, 1 = bf16 hi/lo split, 2 =
 * single-pass f16 with the query's scale exponent q_exp[i] -- NULL = 0 -- and the rows' base_exp) over
 * k_acc columns, of any query with |q|^2 = q_norm2[i] and any row with |b| <= b_max; +inf = no bound.
 * alaya_flat_ip_proven: out[i] = 1 when a k-th reference distance kth_d[i] is proven strictly below
 * every row whose scan value -2 C~ is >= cutoff[i], given slack[i]. */
int alaya_flat_ip_slack(int contraction, uint32_t k_acc, const float *q_norm2, const int *q_exp, uint64_t n,
                        float b_max, int base_exp, float *out);
int alaya_flat_ip_proven(const float *kth_d, const float *cutoff, const float *slack, uint64_t n, uint8_t *out);
/* Which graph-search kernel a request gets, evaluated on the host from the list every launch is
 * planned from (csrc/search_variants.h).  A kernel variant is (space: 0 = f32 rows, 1 / 2 = SQ8 codes
 * in the AVX2 / AVX-512 order; chunks: dim / 32, 0 = the runtime-d kernel; mode: a set of feature bits
 * -- 1 phase stamps, 2 spill-table prefetch check, 4 distance helpers, 8 two waves per SIMD, 16
 * candidate screen).  alaya_search_variant: the variant chosen for a search that wants the features
 * `wanted_mode` (its mode is a subset of them), and in *has_mode the bits 4 / 8 / 16 for which this
 * shape has a kernel at all.  alaya_search_variant_at: row `index` of the list, *count its length. */
int alaya_search_variant(uint32_t dim, int ip, int sq8_order, int generic, uint32_t wanted_mode, int *space,
                         uint32_t *chunks, uint32_t *mode, uint32_t *has_mode);
int alaya_search_variant_at(uint32_t index, int *space, uint32_t *chunks, uint32_t *mode, int *l2_only,
                            uint32_t *count);
/* The last graph search's launch shape: persistent workgroups and searchers (waves) per workgroup --
 * workgroups x waves is the number of queries the launch runs at once (introspection). */
int alaya_index_last_launch(const alaya_index *ix, uint32_t *workgroups, uint32_t *waves_per_group);
/* The rest of that launch's plan: LDS bytes per workgroup, the first-level visited table (log2 slots;
 * compact: 1 = 16-bit slots), resident workgroups per CU, and the scout flags (below; 0 = no scouts). */
int alaya_index_last_plan(const alaya_index *ix, uint32_t *lds_bytes, uint32_t *hash_log2, uint32_t *compact,
                          uint32_t *groups_per_cu, uint32_t *scout);
/* Scout of the screened graph search at d = 768 / 960 (L2, integer screen): in a batch that leaves the
 * second wave per SIMD idle, every searcher wave gets a scout wave in its workgroup, which computes the
 * screen's bounds for the neighbours of the nodes the searcher will probably pop next; the searcher
 * takes them at the pop and skips its screen pass, or runs it as before when they are not there.
 * alaya_index_last_launch then reports two waves per searcher.  Environment ALAYA_SEARCH_SCOUT, read per
 * launch: 0 = off, 1 = on, 2 = on and every hit checked against the searcher's own bounds, unset = the
 * width's default; ALAYA_SEARCH_SCOUT_MISS=1 (diagnostics) lets no answer match, and
 * ALAYA_SEARCH_SCOUT_GRID=n (diagnostics) holds a scouted launch to n workgroups, so each searcher and
 * its scout run several queries one after the other.  Results and counters
 * never depend on either.  alaya_index_scout_stats: of the last graph search, summed over its searchers,
 * the expansions that screened, those that took the scout's bounds, the records the scouts read, and
 * the bounds the check found different (waits for that search; zeros when it had no scouts). */
int alaya_index_scout_stats(alaya_index *ix, uint64_t *expansions, uint64_t *hits, uint64_t *records,
                            uint64_t *mismatches);
/* What a scouted launch asks of its scouts: environment ALAYA_SEARCH_SCOUT_POLICY, read per launch, a mask
 * of 1 = the searcher requests the likely next pop right after the screen (the survivor with the
 * smallest bound, if below the first unchecked entry's distance) and 2 = the scout looks at the
 * requests again when a node's adjacency row has arrived and drops a node that is in neither; other
 * bits are ignored, unset = the width's default.  Ignored without scouts.  Results and counters never
 * depend on it.  alaya_index_scout_policy_stats: the mask the last graph search ran with (0 = no
 * scouts; no wait if only the mask is asked for) and, summed over its searchers, the early requests,
 * those the merge confirmed and the nodes dropped at the second look (waits for that search; zeros
 * when it had no scouts). */
int alaya_index_scout_policy_stats(alaya_index *ix, uint32_t *policy, uint64_t *early_posts, uint64_t *confirmed,
                                   uint64_t *abandoned);
int alaya_index_info(const alaya_index *ix, uint64_t *n, uint32_t *dim, uint32_t *stride,
                     int *metric, uint64_t *device_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ALAYA_HIP_H_ */
