/*
 * TEST INFRASTRUCTURE ONLY -- CPU restatement of the engine's *batched* HNSW construction, the
 * checker for alaya_index_build_graph at batch sizes above one (build_search / build_select /
 * build_apply and the host's batch schedule).  Written from the description in
 * alayalite_amd/csrc/build_kernels.h and DESIGN.md ("Device graph construction"), sharing no code
 * with the product: plain loops, a std::vector<bool> visited set, std::sort.  The batched
 * algorithm is deterministic by construction (phases are separate launches, the reverse edges'
 * sort keys are unique, pool ties are ordered by arrival, prune ties by id), so it has exactly one
 * right answer and this file states it.
 *
 * Levels     the seeded draw of oracle_build.cpp (get_random_level, hnswlib.hpp:182-186), in label
 *            order.  M = R/2, ef = max(ef_construction, M).  Every list is R wide and -1 padded;
 *            its capacity is R on level 0 and M above.
 * Schedule   points enter in label order in batches of max(1, min(max_batch, inserted / batch_div))
 *            (0 = the defaults 16 and 65536); a batch closes at a point whose level exceeds the
 *            graph's max level, and that point becomes the entry point after the batch.  Per batch,
 *            for L = min(top level of the batch, max level) down to 0, one step over the active
 *            points (min(level, max level) >= L); then `refine` more steps on level 0 unless the
 *            batch is a single point.  The graph is frozen within a step:
 *              1. every active point searches level L                 -> candidate pool
 *              2. every active point selects                          -> own row, next, reverse edges
 *              3. every destination of a reverse edge applies its incoming edges.
 * Search     entry = greedy descent from ep through the levels above L (first index of a list's
 *            minimum, taken only when strictly below the current distance) when L is the point's
 *            first level and the step is no refine step, else next[point].  The entry and the point
 *            itself start visited.  Pool = LinearPool (orc_pool_*, oracle.cpp) of capacity ef; fresh
 *            neighbours are inserted in row order; a row ends at its first -1; the loop runs while
 *            an unexpanded entry remains.
 * Selection  getNeighborsByHeuristic2 over the pool in ascending order, up to M kept (all of them if
 *            the pool holds fewer than M).  Own row = the kept ids farthest first, -1 across the
 *            rest of the width.  next = closest kept (ep if none).  One reverse edge (kept, point,
 *            distance) per kept candidate.
 * Apply      per destination v: incoming points in ascending id, in groups of 64.  Within a group,
 *            points the list held at the group's start are dropped, the rest appended; if the count
 *            then exceeds the capacity: sort by (distance to v, id), heuristic to the capacity,
 *            store farthest first.  The row is rewritten only if something was appended.
 * Counters   prunes: destinations pruned at least once in a step; appends: appended points of the
 *            destinations never pruned in that step; heuristic_dists: every distance evaluated
 *            outside the searches (per candidate tested, the number kept so far; in apply also the
 *            existing list's count when count + incoming exceeds the capacity).
 */
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <random>
#include <thread>
#include <vector>

#include "oracle.h"

namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr size_t kGroup = 64;  // apply: incoming points taken per group

struct Cand {
  uint32_t id;
  float d;
};

struct Edge {
  uint32_t to, from;
  float d;
};

class BatchedBuild {
 public:
  BatchedBuild(const float *rows, uint64_t n, uint32_t dim, int metric, int generic, uint32_t R, uint32_t efc,
               uint64_t seed)
      : rows_(rows), n_(n), dim_(dim), metric_(metric), generic_(generic), R_(R), M_(R / 2),
        ef_(std::max(efc, R / 2)), level_(n, 0), off_(n, 0) {
    // get_random_level (hnswlib.hpp:182-186) with mult = 1 / ln(M); M = 1 makes every draw
    // infinite, whose truncation is left at level 0
    std::default_random_engine gen;
    gen.seed(seed);
    const double mult = 1.0 / std::log(1.0 * static_cast<double>(M_));
    uint64_t slots = 0;
    for (uint64_t i = 0; i < n_; ++i) {
      std::uniform_real_distribution<double> u(0.0, 1.0);
      const double r = -std::log(u(gen)) * mult;
      level_[i] = std::isfinite(r) ? static_cast<uint32_t>(static_cast<size_t>(r)) : 0u;
      off_[i] = slots;
      slots += static_cast<uint64_t>(level_[i]) * R_;
    }
    l0_.assign(n_ * R_, kNone);
    upper_.assign(slots, kNone);
  }

  void run(uint32_t batch_div, uint32_t max_batch, uint32_t refine) {
    batch_div = batch_div ? batch_div : 16;
    max_batch = max_batch ? max_batch : 65536;
    ep_ = 0;
    maxl_ = n_ ? static_cast<int>(level_[0]) : 0;
    max_batch_seen_ = 1;
    uint64_t i = 1;
    while (i < n_) {
      const uint64_t b = std::max<uint64_t>(1, std::min<uint64_t>(max_batch, i / batch_div));
      uint64_t end = std::min<uint64_t>(n_, i + b);
      int top = 0;
      for (uint64_t j = i; j < end; ++j) {
        top = std::max(top, std::min(static_cast<int>(level_[j]), maxl_));
        if (static_cast<int>(level_[j]) > maxl_) {  // raises the max level: closes the batch
          end = j + 1;
          break;
        }
      }
      ++batches_;
      first_ = static_cast<uint32_t>(i);
      next_.assign(end - i, 0u);
      for (int L = top; L >= 0; --L) step(i, end, L, false);
      if (end - i > 1)
        for (uint32_t r = 0; r < refine; ++r) step(i, end, 0, true);
      if (static_cast<int>(level_[end - 1]) > maxl_) {
        ep_ = static_cast<uint32_t>(end - 1);
        maxl_ = static_cast<int>(level_[end - 1]);
      }
      i = end;
    }
  }

  void export_graph(uint32_t *l0, uint32_t *levels, uint64_t *upper_off, uint32_t *upper_edges, uint32_t *ep,
                    uint64_t *stats) const {
    std::copy(l0_.begin(), l0_.end(), l0);
    std::copy(level_.begin(), level_.end(), levels);
    std::copy(off_.begin(), off_.end(), upper_off);
    std::copy(upper_.begin(), upper_.end(), upper_edges);
    *ep = ep_;
    stats[0] = batches_;
    stats[1] = max_batch_seen_;
    stats[2] = static_cast<uint64_t>(maxl_);
    stats[3] = prunes_;
    stats[4] = appends_;
    stats[5] = heuristic_dists_;
    stats[6] = max_incoming_;
    stats[7] = steps_;
  }

  uint64_t upper_slots() const { return upper_.size(); }

 private:
  float dist(uint32_t a, uint32_t b) const {
    const float *x = rows_ + static_cast<uint64_t>(a) * dim_;
    const float *y = rows_ + static_cast<uint64_t>(b) * dim_;
    if (generic_) return metric_ == ORC_L2 ? orc_l2_generic(x, y, dim_, 0) : orc_ip_generic(x, y, dim_, 0);
    return metric_ == ORC_L2 ? orc_l2_f32(x, y, dim_) : orc_ip_f32(x, y, dim_);
  }

  uint32_t *row(uint32_t u, int level) {
    return level == 0 ? &l0_[static_cast<uint64_t>(u) * R_] : &upper_[off_[u] + static_cast<uint64_t>(level - 1) * R_];
  }
  const uint32_t *row(uint32_t u, int level) const { return const_cast<BatchedBuild *>(this)->row(u, level); }
  uint32_t row_count(const uint32_t *r) const {  // ids before the first -1
    uint32_t c = 0;
    while (c < R_ && r[c] != kNone) ++c;
    return c;
  }

  // Work items of one phase are independent (each writes only its own row, pool or tally), so they
  // are spread over a few threads; the result does not depend on how.
  template <typename F>
  static void for_each_item(size_t n, F f) {
    const size_t nt = std::min<size_t>({16, std::max(1u, std::thread::hardware_concurrency()), n / 4});
    if (nt < 2) {
      for (size_t i = 0; i < n; ++i) f(i);
      return;
    }
    std::atomic<size_t> at{0};
    std::vector<std::thread> ts;
    for (size_t t = 0; t < nt; ++t)
      ts.emplace_back([&] {
        for (size_t i = at.fetch_add(1); i < n; i = at.fetch_add(1)) f(i);
      });
    for (std::thread &t : ts) t.join();
  }

  struct Tally {  // what one select or one apply adds to the counters
    uint64_t dists = 0, appended = 0, incoming = 0;
    bool pruned = false;
  };

  // one level of one batch: search all, then select all, then apply per destination
  void step(uint64_t begin, uint64_t end, int L, bool refine) {
    std::vector<uint32_t> active;
    for (uint64_t j = begin; j < end; ++j)
      if (std::min(static_cast<int>(level_[j]), maxl_) >= L) active.push_back(static_cast<uint32_t>(j));
    ++steps_;
    max_batch_seen_ = std::max<uint64_t>(max_batch_seen_, active.size());
    std::vector<std::vector<Cand>> pools(active.size());
    for_each_item(active.size(), [&](size_t a) { pools[a] = search(active[a], L, refine); });
    std::vector<std::vector<Edge>> out(active.size());
    std::vector<Tally> sel(active.size());
    for_each_item(active.size(), [&](size_t a) { select(active[a], L, pools[a], out[a], sel[a]); });
    std::vector<Edge> edges;
    for (size_t a = 0; a < active.size(); ++a) {
      edges.insert(edges.end(), out[a].begin(), out[a].end());
      heuristic_dists_ += sel[a].dists;
    }
    std::sort(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) {
      return x.to < y.to || (x.to == y.to && x.from < y.from);
    });
    std::vector<size_t> seg;  // start of every destination's run of edges, then the end
    for (size_t s = 0; s < edges.size(); ++s)
      if (s == 0 || edges[s].to != edges[s - 1].to) seg.push_back(s);
    seg.push_back(edges.size());
    std::vector<Tally> app(seg.size() - 1);
    for_each_item(app.size(), [&](size_t g) { apply(edges[seg[g]].to, L, &edges[seg[g]], seg[g + 1] - seg[g], app[g]); });
    for (const Tally &t : app) {
      heuristic_dists_ += t.dists;
      prunes_ += t.pruned ? 1 : 0;
      appends_ += t.pruned ? 0 : t.appended;
      max_incoming_ = std::max(max_incoming_, t.incoming);
    }
  }

  std::vector<Cand> search(uint32_t pt, int L, bool refine) const {
    const int top = std::min(static_cast<int>(level_[pt]), maxl_);
    const bool descend = top == L && !refine;
    uint32_t u = descend ? ep_ : next_[pt - first_];
    float cur = dist(pt, u);
    if (descend) {
      for (int level = maxl_; level > L; --level) {
        for (bool changed = true; changed;) {
          changed = false;
          const uint32_t *list = row(u, level);
          const uint32_t cnt = row_count(list);
          uint32_t best = kNone;
          float mn = 0.f;
          for (uint32_t j = 0; j < cnt; ++j) {
            const float d = dist(pt, list[j]);
            if (best == kNone || d < mn) {  // first index of the minimum
              best = list[j];
              mn = d;
            }
          }
          if (best != kNone && mn < cur) {
            u = best;
            cur = mn;
            changed = true;
          }
        }
      }
    }
    std::vector<bool> visited(n_, false);
    orc_pool *pool = orc_pool_new(0, static_cast<int>(ef_));
    orc_pool_insert(pool, u, cur);
    visited[u] = true;
    visited[pt] = true;
    while (orc_pool_has_next(pool)) {
      const uint32_t x = orc_pool_pop(pool);
      const uint32_t *list = row(x, L);
      for (uint32_t j = 0; j < R_ && list[j] != kNone; ++j) {
        const uint32_t v = list[j];
        if (visited[v]) continue;
        visited[v] = true;
        orc_pool_insert(pool, v, dist(pt, v));
      }
    }
    std::vector<Cand> out(orc_pool_size(pool));
    for (size_t k = 0; k < out.size(); ++k) out[k] = Cand{orc_pool_id(pool, k), orc_pool_dist(pool, k)};
    orc_pool_free(pool);
    return out;
  }

  // getNeighborsByHeuristic2 over candidates in ascending order; kept in ascending order
  std::vector<Cand> heuristic(const std::vector<Cand> &cand, size_t m, uint64_t &n_dist) const {
    if (cand.size() < m) return cand;
    std::vector<Cand> kept;
    for (size_t k = 0; k < cand.size() && kept.size() < m; ++k) {
      bool good = true;
      for (const Cand &s : kept)
        if (dist(cand[k].id, s.id) < cand[k].d) good = false;  // every kept one is evaluated
      n_dist += kept.size();
      if (good) kept.push_back(cand[k]);
    }
    return kept;
  }

  void select(uint32_t pt, int L, const std::vector<Cand> &pool, std::vector<Edge> &edges, Tally &t) {
    const std::vector<Cand> kept = heuristic(pool, M_, t.dists);
    uint32_t *own = row(pt, L);
    for (uint32_t j = 0; j < R_; ++j) own[j] = j < kept.size() ? kept[kept.size() - 1 - j].id : kNone;
    next_[pt - first_] = kept.empty() ? ep_ : kept[0].id;
    for (const Cand &c : kept) edges.push_back(Edge{c.id, pt, c.d});
  }

  void apply(uint32_t v, int L, const Edge *in, size_t n_in, Tally &t) {
    const size_t cap = L == 0 ? R_ : M_;
    uint32_t *list = row(v, L);
    std::vector<Cand> cur(row_count(list));
    for (size_t k = 0; k < cur.size(); ++k) cur[k] = Cand{list[k], 0.f};
    if (cur.size() + n_in > cap) {  // a prune is possible: the existing list's distances
      for (Cand &c : cur) c.d = dist(v, c.id);
      t.dists += cur.size();
    }
    t.incoming = n_in;
    for (size_t pos = 0; pos < n_in; pos += kGroup) {
      const size_t held = cur.size();
      for (size_t k = pos; k < std::min(n_in, pos + kGroup); ++k) {
        bool fresh = true;
        for (size_t h = 0; h < held; ++h) fresh = fresh && cur[h].id != in[k].from;
        if (!fresh) continue;
        cur.push_back(Cand{in[k].from, in[k].d});
        ++t.appended;
      }
      if (cur.size() <= cap) continue;
      std::sort(cur.begin(), cur.end(), [](const Cand &a, const Cand &b) {
        return a.d < b.d || (a.d == b.d && a.id < b.id);
      });
      cur = heuristic(cur, cap, t.dists);
      std::reverse(cur.begin(), cur.end());  // farthest first
      t.pruned = true;
    }
    if (t.appended)
      for (uint32_t j = 0; j < R_; ++j) list[j] = j < cur.size() ? cur[j].id : kNone;
  }

  const float *rows_;
  uint64_t n_;
  uint32_t dim_;
  int metric_, generic_;
  uint32_t R_, M_, ef_;
  std::vector<uint32_t> level_;
  std::vector<uint64_t> off_;
  std::vector<uint32_t> l0_, upper_;
  std::vector<uint32_t> next_;  // batch-local: entry of a point's next step
  uint32_t first_ = 0;          // first point of the current batch
  uint32_t ep_ = 0;
  int maxl_ = 0;
  uint64_t batches_ = 0, steps_ = 0, max_batch_seen_ = 1, prunes_ = 0, appends_ = 0, heuristic_dists_ = 0,
           max_incoming_ = 0;
};

}  // namespace

struct orc_hnsw_batched {
  BatchedBuild b;
};

extern "C" {

orc_hnsw_batched *orc_hnsw_batched_build(const float *rows, uint64_t n, uint32_t dim, int metric, int generic,
                                         uint32_t R, uint32_t ef_construction, uint64_t seed, uint32_t batch_div,
                                         uint32_t max_batch, uint32_t refine) {
  auto *o = new orc_hnsw_batched{BatchedBuild(rows, n, dim, metric, generic, R, ef_construction, seed)};
  o->b.run(batch_div, max_batch, refine);
  return o;
}

uint64_t orc_hnsw_batched_upper_slots(const orc_hnsw_batched *o) { return o->b.upper_slots(); }

void orc_hnsw_batched_export(const orc_hnsw_batched *o, uint32_t *l0, uint32_t *levels, uint64_t *upper_off,
                             uint32_t *upper_edges, uint32_t *ep, uint64_t *stats) {
  o->b.export_graph(l0, levels, upper_off, upper_edges, ep, stats);
}

void orc_hnsw_batched_free(orc_hnsw_batched *o) { delete o; }

}  // extern "C"
