// _alayalitepy: pybind11 module with the reference binding's surface (python/src/pybind.cpp:37-147)
// -- IndexType / MetricType / QuantizationType enums, IndexParams, PyIndexInterface -- implemented
// over the C ABI of libalaya_hip.so (include/alaya_hip.h).  All search work runs on the MI355X;
// there is no CPU search path: construction fails loudly when no HIP device is present.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <memory>
#include <queue>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/alaya_hip.h"

extern "C" int alaya_index_flat_diag(alaya_index *, const float *, uint64_t, uint32_t, int, uint32_t *, float *,
                                     uint32_t *, uint32_t *, void *);
#include "host_distance.h"

namespace py = pybind11;

namespace alaya_py {

// include/index/index_type.hpp:27-33, include/utils/metric_type.hpp, quantization_type.hpp
enum class IndexType { FLAT = 0, HNSW = 1, NSG = 2, FUSION = 3, QG = 4 };
enum class MetricType { L2 = 0, IP = 1, COS = 2, NONE = 3 };
enum class QuantizationType { NONE = 0, SQ8 = 1, SQ4 = 2, RABITQ = 3 };

// python/include/params.hpp:29-52 (max_nbrs_ is not exposed by the reference binding either)
struct IndexParams {
  IndexType index_type_ = IndexType::HNSW;
  py::dtype data_type_ = py::dtype::of<float>();
  py::dtype id_type_ = py::dtype::of<uint32_t>();
  QuantizationType quantization_type_ = QuantizationType::NONE;
  MetricType metric_ = MetricType::L2;
  uint32_t capacity_ = 100000;
  uint32_t max_nbrs_ = 32;
};

void check(int rc) {
  if (rc == ALAYA_OK) return;
  const std::string msg = alaya_last_error();
  if (rc == ALAYA_ERR_ARG) throw py::value_error(msg);
  throw std::runtime_error(msg);
}

// numpy arguments as C-contiguous arrays of one element type, converted on the way in where need be
template <typename T>
using CArray = py::array_t<T, py::array::c_style | py::array::forcecast>;
using F32Array = CArray<float>;
using U32Array = CArray<uint32_t>;
using U8Array = CArray<uint8_t>;

// "no row" as a 64-bit id: an empty result slot (widen_ids), alaya_index_insert on a full index
constexpr uint64_t kNoId64 = UINT64_MAX;

template <typename T>
py::array_t<T> out2d(uint64_t rows, uint64_t cols) {
  return py::array_t<T>({static_cast<py::ssize_t>(rows), static_cast<py::ssize_t>(cols)});
}

// a device address (or stream handle) handed over as an integer, e.g. torch's data_ptr()
template <typename T>
T *dptr(uintptr_t p) {
  return reinterpret_cast<T *>(p);
}

// The filtered calls' masks: allow_words uint32 [n_masks, ceil(n / 32)] over n rows, and mask_of_query, each of
// the nq queries' mask or None (the C call then accepts one mask only).  `indices` owns what of_query points to.
struct Masks {
  const uint32_t *words = nullptr;
  uint32_t n_masks = 0;
  const uint32_t *of_query = nullptr;
  U32Array indices;
};

Masks parse_masks(const U32Array &allow_words, const py::object &mask_of_query, uint64_t n, uint64_t nq) {
  if (allow_words.ndim() != 2 || static_cast<uint64_t>(allow_words.shape(1)) != (n + 31) / 32 || allow_words.shape(0) < 1)
    throw py::value_error("allow_words must be uint32 [n_masks, ceil(n / 32)]");
  Masks m;
  m.words = allow_words.data();
  m.n_masks = static_cast<uint32_t>(allow_words.shape(0));
  if (!mask_of_query.is_none()) {
    m.indices = U32Array(mask_of_query);
    if (m.indices.ndim() != 1 || static_cast<uint64_t>(m.indices.shape(0)) != nq)
      throw py::value_error("mask_of_query must hold one index per query");
    m.of_query = m.indices.data();
  }
  return m;
}

// The range calls' masks: allow_words None = no mask (mask_of_query must then be None too), else parse_masks.
// `words` owns what the result's words point to.
Masks parse_range_masks(const py::object &allow_words, U32Array &words, const py::object &mask_of_query, uint64_t n,
                        uint64_t nq) {
  if (allow_words.is_none()) {
    if (!mask_of_query.is_none()) throw py::value_error("mask_of_query needs allow_words");
    return Masks{};
  }
  words = U32Array(allow_words);
  return parse_masks(words, mask_of_query, n, nq);
}

// The range calls' radius, a number or an array of shape (nq,), as nq f32 values.
std::vector<float> parse_radii(const py::object &radius, uint64_t nq) {
  const F32Array a(radius);
  if (a.ndim() == 0) return std::vector<float>(nq, *a.data());
  if (a.ndim() != 1 || static_cast<uint64_t>(a.shape(0)) != nq)
    throw py::value_error("radius must be a number or hold one value per query");
  return std::vector<float>(a.data(), a.data() + nq);
}

enum DType { kF32 = 0, kI8, kU8, kF64, kI32, kU32 };

DType dtype_code(const py::dtype &dt) {
  if (dt.is(py::dtype::of<float>())) return kF32;
  if (dt.is(py::dtype::of<int8_t>())) return kI8;
  if (dt.is(py::dtype::of<uint8_t>())) return kU8;
  if (dt.is(py::dtype::of<double>())) return kF64;
  if (dt.is(py::dtype::of<int32_t>())) return kI32;
  if (dt.is(py::dtype::of<uint32_t>())) return kU32;
  throw std::runtime_error("Unsupported data type");  // dispatch.hpp: "Unsupported data type"
}

size_t dtype_size(DType t) {
  switch (t) {
    case kF32: case kI32: case kU32: return 4;
    case kI8: case kU8: return 1;
    case kF64: return 8;
  }
  return 4;
}

// DataType -> float as the reference's generic l2_sqr<T>/ip_sqr<T> casts each element
// (distance_l2.ipp:735-741).  For float32 data this is the identity.
void to_float(const void *src, DType t, size_t count, float *dst) {
  switch (t) {
    case kF32: std::memcpy(dst, src, count * 4); break;
    case kI8: for (size_t i = 0; i < count; ++i) dst[i] = static_cast<const int8_t *>(src)[i]; break;
    case kU8: for (size_t i = 0; i < count; ++i) dst[i] = static_cast<const uint8_t *>(src)[i]; break;
    case kF64: for (size_t i = 0; i < count; ++i) dst[i] = static_cast<float>(static_cast<const double *>(src)[i]); break;
    case kI32: for (size_t i = 0; i < count; ++i) dst[i] = static_cast<float>(static_cast<const int32_t *>(src)[i]); break;
    case kU32: for (size_t i = 0; i < count; ++i) dst[i] = static_cast<float>(static_cast<const uint32_t *>(src)[i]); break;
  }
}

// get_l2_sqr_sq8_func / get_ip_sqr_sq8_func pick the AVX-512 kernel on AVX-512F hosts, else AVX2
// (distance_l2.ipp:694-708): the device reproduces the order this host's reference build uses.
int host_sq8_order() { return __builtin_cpu_supports("avx512f") ? 2 : 1; }

// A host graph's arrays: (n x R l0, levels, upper_off, upper_edges, ep, upper_R, eps); levels and upper_off
// are None for a graph without overlay.
py::tuple graph_arrays_of(const alaya_graph *g) {
  uint64_t n, nue;
  uint32_t R, upper_R, ep, max_level, n_eps;
  int has_overlay;
  check(alaya_graph_info(g, &n, &R, &has_overlay, &upper_R, &ep, &max_level, &nue, &n_eps));
  py::array_t<uint32_t> l0 = out2d<uint32_t>(n, R);
  py::array_t<uint32_t> levels(static_cast<py::ssize_t>(has_overlay ? n : 0));
  py::array_t<uint64_t> off(static_cast<py::ssize_t>(has_overlay ? n : 0));
  py::array_t<uint32_t> ue(static_cast<py::ssize_t>(nue));
  py::array_t<uint32_t> eps(static_cast<py::ssize_t>(n_eps));
  check(alaya_graph_export(g, l0.mutable_data(), levels.mutable_data(), off.mutable_data(), ue.mutable_data(),
                           eps.mutable_data()));
  return py::make_tuple(l0, has_overlay ? py::object(levels) : py::none(), has_overlay ? py::object(off) : py::none(), ue,
                        ep, upper_R, eps);
}

// The launch controls and the device counters of the last search, as both index classes expose them.
class LaunchControls {
 public:
  void set_hash_log2(uint32_t v) { check(alaya_index_set_hash_log2(ix_, v)); }
  void set_visited_mode(int m) { check(alaya_index_set_visited_mode(ix_, m)); }
  void set_helpers(int m) { check(alaya_index_set_helpers(ix_, m)); }
  py::tuple last_launch() {
    uint32_t g = 0, w = 0;
    check(alaya_index_last_launch(ix_, &g, &w));
    return py::make_tuple(g, w);
  }
  py::tuple help_stats() {
    uint64_t m = 0, x = 0, r = 0;
    check(alaya_index_help_stats(ix_, &m, &x, &r));
    return py::make_tuple(m, x, r);
  }
  py::tuple screen_stats() {
    uint64_t a = 0, b = 0;
    check(alaya_index_screen_stats(ix_, &a, &b));
    return py::make_tuple(a, b);
  }
  py::tuple scout_stats() {
    uint64_t e = 0, h = 0, r = 0, m = 0;
    check(alaya_index_scout_stats(ix_, &e, &h, &r, &m));
    return py::make_tuple(e, h, r, m);
  }
  py::tuple scout_policy_stats() {
    uint64_t a = 0, c = 0, d = 0;
    check(alaya_index_scout_policy_stats(ix_, nullptr, &a, &c, &d));
    return py::make_tuple(a, c, d);
  }
  uint32_t scout_policy() {
    uint32_t pol = 0;
    check(alaya_index_scout_policy_stats(ix_, &pol, nullptr, nullptr, nullptr));
    return pol;
  }
  py::dict last_plan() {
    uint32_t g = 0, w = 0, lds = 0, hl = 0, c = 0, pc = 0, sc = 0;
    check(alaya_index_last_launch(ix_, &g, &w));
    check(alaya_index_last_plan(ix_, &lds, &hl, &c, &pc, &sc));
    py::dict d;
    d["workgroups"] = g;
    d["waves_per_group"] = w;
    d["lds_bytes"] = lds;
    d["hash_log2"] = hl;
    d["compact"] = c != 0;
    d["groups_per_cu"] = pc;
    d["scout"] = sc;
    d["scout_policy"] = scout_policy();
    return d;
  }

 protected:
  alaya_index *ix_ = nullptr;
};

class PyIndexInterface : public LaunchControls {
 public:
  explicit PyIndexInterface(const IndexParams &params) : params_(params) {
    dtype_ = dtype_code(params_.data_type_);
    if (params_.id_type_.is(py::dtype::of<uint32_t>())) {
      id_bytes_ = 4;
    } else if (params_.id_type_.is(py::dtype::of<uint64_t>())) {
      id_bytes_ = 8;
    } else {
      throw std::runtime_error("Unsupported id type");
    }
    if (params_.quantization_type_ == QuantizationType::SQ4 ||
        params_.quantization_type_ == QuantizationType::RABITQ)
      throw std::runtime_error("quantization type not supported by the MI355X engine (SQ4/RaBitQ are out of scope)");
    if (params_.metric_ == MetricType::COS && dtype_ != kF32 && dtype_ != kF64) {
      throw std::runtime_error("COS metric only support float or double");  // raw_space.hpp:88-93
    }
    // SQ8 over a non-float DataType takes the reference's generic SQ8 branch (distance_l2.ipp:750-763,
    // quantize in double arithmetic for double data, sq8.hpp:118-130), which the device does not
    // implement: refuse rather than return different neighbours.
    if (params_.quantization_type_ == QuantizationType::SQ8 && dtype_ != kF32)
      throw std::runtime_error("SQ8 quantization of non-float32 data is not supported by the MI355X engine");
    check(alaya_index_create(0, &ix_));
  }
  ~PyIndexInterface() {
    if (graph_) alaya_graph_free(graph_);
    if (ix_) alaya_index_destroy(ix_);
  }
  PyIndexInterface(const PyIndexInterface &) = delete;
  PyIndexInterface &operator=(const PyIndexInterface &) = delete;

  std::string to_string() const { return "PyIndexInterface"; }

  // PyIndex::fit (index.hpp:177-227)
  // builder: "host" = HNSWBuilder restated on the host (num_threads == 1 reproduces the reference's
  // sequential graph exactly); "gpu" = batched insertion on the device (alaya_index_build_graph).
  void fit(py::array vectors, uint32_t ef_construction, uint32_t num_threads, const std::string &builder) {
    if (builder != "host" && builder != "gpu") throw py::value_error("builder must be 'host' or 'gpu'");
    if (vectors.ndim() != 2) throw std::runtime_error("Array must be 2D");
    check_dtype(vectors);
    py::array arr = py::array::ensure(vectors, py::array::c_style);
    const uint64_t n = arr.shape(0);
    dim_ = static_cast<uint32_t>(arr.shape(1));
    // RawSpace::fit silently stops storing past capacity (sequential_storage.hpp:77-80); the
    // builder (and the search bitset) still see n items.  Keep it defined: refuse instead.
    if (n > params_.capacity_) throw std::runtime_error("number of vectors exceeds the index capacity");
    // COS normalises the caller's rows in place (raw_space.hpp:131-140) -- done identically here.
    if (params_.metric_ == MetricType::COS) normalize_in_place(arr, n);
    raw_.assign(static_cast<const char *>(arr.data()),
                static_cast<const char *>(arr.data()) + n * dim_ * dtype_size(dtype_));
    n_ = n;
    delete_cnt_ = 0;
    valid_.clear();
    rows_f32_.resize(n * dim_);
    to_float(raw_.data(), dtype_, n * dim_, rows_f32_.data());
    if (graph_) alaya_graph_free(graph_);
    graph_ = nullptr;
    if (builder == "gpu") {
      {
        py::gil_scoped_release nogil;
        check(alaya_index_set_base(ix_, rows_f32_.data(), n, dim_, dist_code(), nullptr));
        uint64_t st[8] = {0};
        check(alaya_index_build_graph(ix_, params_.max_nbrs_, ef_construction, 100, 0, 0, 2, &graph_, st));
        last_build_us_ = st[5];
      }
      if (params_.quantization_type_ == QuantizationType::SQ8) {
        train_sq8(num_threads);
        check(alaya_index_set_sq8(ix_, sq_codes_.data(), n_, dim_, sq_min_.data(), sq_max_.data(), host_sq8_order()));
      }
      updates_enabled_ = false;
      graph_dirty_ = false;
      return;
    }
    {
      py::gil_scoped_release nogil;
      check(alaya_graph_build_hnsw(rows_f32_.data(), n, dim_, dist_code(), params_.max_nbrs_,
                                   ef_construction, num_threads, 100, &graph_));
    }
    if (params_.quantization_type_ == QuantizationType::SQ8) train_sq8(num_threads);
    upload();
  }

  py::array search(py::array query, uint32_t topk, uint32_t ef) {
    if (query.ndim() != 1) throw std::runtime_error("query must be 1D");
    py::array q2 = query.attr("reshape")(1, query.shape(0));
    auto r = run(q2, topk, ef, false);
    return r.first.attr("reshape")(topk);
  }

  py::array batch_search(py::array queries, uint32_t topk, uint32_t ef, uint32_t /*num_threads*/) {
    return run(queries, topk, ef, false).first;
  }

  py::object batch_search_with_distance(py::array queries, uint32_t topk, uint32_t ef,
                                        uint32_t /*num_threads*/) {
    auto r = run(queries, topk, ef, true);
    return py::make_tuple(r.first, r.second);
  }

  // --- extra (not in the reference binding): the exact top-k over the index's own device rows (the
  // flat search: every valid row, the index's metric, ties by id) -- what a recall measurement of
  // batch_search at some ef needs.  Empty slots hold (the id type's maximum, FLT_MAX).
  py::object exact_search(py::array queries, uint32_t topk) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    py::array q = prepare_queries(queries);
    const uint64_t nq = q.shape(0);
    std::vector<uint32_t> ids32(nq * topk);
    py::array_t<float> dists = out2d<float>(nq, topk);
    {
      py::gil_scoped_release nogil;
      check(alaya_index_flat_search(ix_, static_cast<const float *>(q.data()), nq, topk, ids32.data(),
                                    dists.mutable_data(), nullptr));
    }
    return py::make_tuple(widen_ids(ids32, nq, topk, true), dists);
  }

  // --- extra (not in the reference binding): the topk nearest rows among those a mask allows
  // (alaya_index_filtered_search).  allow_words: uint32 [n_masks, ceil(n / 32)] (utils.pack_allow);
  // mask_of_query: each query's mask, or None with one mask.  Empty slots as exact_search's.
  // SQ8 indexes run alaya_index_filtered_search_sq8 with batch_search's two query forms; pool: its
  // candidate pool (0 = the default), which an unquantized index does not have.  through: the traversal
  // that steps through disallowed neighbours (alaya_index_filtered_search_hop; f32 indexes only), whose rows
  // stepped through per query last_through() then holds.
  py::object filtered_search(py::array queries, uint32_t topk, uint32_t ef, U32Array allow_words,
                             py::object mask_of_query, uint32_t pool, bool through) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    const bool sq8 = params_.quantization_type_ == QuantizationType::SQ8;
    if (through && (sq8 || pool != 0)) throw py::value_error("the through traversal searches f32 indexes only");
    if (!sq8 && params_.quantization_type_ != QuantizationType::NONE)
      throw std::runtime_error("filtered_search: the MI355X engine has float32 and SQ8 indexes only");
    if (!sq8 && pool != 0) throw py::value_error("pool applies to SQ8 indexes only");
    py::array q = prepare_queries(queries);
    const uint64_t nq = q.shape(0);
    const Masks m = parse_masks(allow_words, mask_of_query, n_, nq);
    std::vector<uint32_t> ids32(nq * topk);
    py::array_t<float> dists = out2d<float>(nq, topk);
    last_counters_.assign(nq * 4, 0);
    last_through_.assign(through ? nq : 0, 0);
    const float *qp = static_cast<const float *>(q.data());
    if (sq8) {
      // the traversal encodes the query as given, the rerank's f32 distance takes the normalised one (run())
      const float *sq = raw_queries_.empty() ? qp : raw_queries_.data();
      py::gil_scoped_release nogil;
      check(alaya_index_filtered_search_sq8(ix_, sq, qp, nq, topk, ef, pool, m.words, m.n_masks, m.of_query, ids32.data(),
                                            dists.mutable_data(), last_counters_.data()));
    } else if (through) {
      py::gil_scoped_release nogil;
      check(alaya_index_filtered_search_hop(ix_, qp, nq, topk, ef, m.words, m.n_masks, m.of_query, ids32.data(),
                                            dists.mutable_data(), last_counters_.data(), last_through_.data()));
    } else {
      py::gil_scoped_release nogil;
      check(alaya_index_filtered_search(ix_, qp, nq, topk, ef, m.words, m.n_masks, m.of_query, ids32.data(),
                                        dists.mutable_data(), last_counters_.data()));
    }
    return py::make_tuple(widen_ids(ids32, nq, topk, true), dists);
  }

  // --- extra (not in the reference binding): exact_search over the rows a mask allows
  // (alaya_index_flat_search_filtered: a scan of the allowed valid rows, for small allowed shares).
  // allow_words / mask_of_query as for filtered_search; the query forms and the empty slots are
  // exact_search's.  An SQ8 index is scanned on its f32 rows.
  py::object exact_search_filtered(py::array queries, uint32_t topk, U32Array allow_words, py::object mask_of_query) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    py::array q = prepare_queries(queries);
    const uint64_t nq = q.shape(0);
    const Masks m = parse_masks(allow_words, mask_of_query, n_, nq);
    std::vector<uint32_t> ids32(nq * topk);
    py::array_t<float> dists = out2d<float>(nq, topk);
    {
      py::gil_scoped_release nogil;
      check(alaya_index_flat_search_filtered(ix_, static_cast<const float *>(q.data()), nq, topk, m.words, m.n_masks,
                                             m.of_query, ids32.data(), dists.mutable_data()));
    }
    return py::make_tuple(widen_ids(ids32, nq, topk, true), dists);
  }

  // --- extra (not in the reference binding): every valid (and, with masks, allowed) row within `radius` (a
  // number or one per query) of the query, by an exact scan of the rows (alaya_index_flat_range_search).
  // Returns (counts[nq], ids[nq, max_results], dists[nq, max_results]): counts are exact and not capped, row i
  // holds min(counts[i], max_results) hits by (distance, id) -- the ones with the smallest ids when there are
  // more -- then empty slots as exact_search's.  The query forms are exact_search's; allow_words /
  // mask_of_query as for range_search.  An SQ8 index is scanned on its f32 rows.
  py::object exact_range_search(py::array queries, py::object radius, uint32_t max_results, py::object allow_words,
                                py::object mask_of_query) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    py::array q = prepare_queries(queries);
    const uint64_t nq = q.shape(0);
    U32Array words;
    const Masks m = parse_range_masks(allow_words, words, mask_of_query, n_, nq);
    const std::vector<float> radii = parse_radii(radius, nq);
    if (max_results == 0 || max_results > 4096) throw py::value_error("max_results must be in 1..4096");
    std::vector<uint32_t> ids32(nq * max_results);
    py::array_t<float> dists = out2d<float>(nq, max_results);
    py::array_t<uint32_t> counts(static_cast<py::ssize_t>(nq));
    uint32_t *cp = counts.mutable_data();
    float *dp = dists.mutable_data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_flat_range_search(ix_, static_cast<const float *>(q.data()), nq, radii.data(), max_results, m.words,
                                          m.n_masks, m.of_query, cp, ids32.data(), dp));
    }
    return py::make_tuple(counts, widen_ids(ids32, nq, max_results, true), dists);
  }

  // --- extra (not in the reference binding): every row the traversal of batch_search at `ef` measures within
  // `radius` (a number or one per query) of the query (alaya_index_range_search; f32 indexes only).  Returns
  // (counts[nq], ids[nq, max_results], dists[nq, max_results], counters[nq, 4]): row i holds its first
  // min(counts[i], max_results) hits to arrive, by (distance, id), then empty slots as exact_search's.
  // allow_words / mask_of_query as for filtered_search, or None for no mask.  radius_mode: the traversal then
  // keeps expanding the in-radius rows it measured (alaya_index_range_search_radius; max_frontier 1..16384 of them
  // per query), and last_range_more() holds (frontier, more_dist) per query.
  py::object range_search(py::array queries, uint32_t ef, py::object radius, uint32_t max_results, py::object allow_words,
                          py::object mask_of_query, bool radius_mode, uint32_t max_frontier, bool more_append) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    if (params_.quantization_type_ != QuantizationType::NONE)
      throw py::value_error("range_search searches f32 indexes only (no SQ8 codes)");
    py::array q = prepare_queries(queries);
    const uint64_t nq = q.shape(0);
    U32Array words;
    const Masks m = parse_range_masks(allow_words, words, mask_of_query, n_, nq);
    const std::vector<float> radii = parse_radii(radius, nq);
    if (max_results == 0 || max_results > 4096) throw py::value_error("max_results must be in 1..4096");
    if (radius_mode && (max_frontier == 0 || max_frontier > 16384))
      throw py::value_error("max_frontier must be in 1..16384");
    std::vector<uint32_t> ids32(nq * max_results);
    py::array_t<float> dists = out2d<float>(nq, max_results);
    py::array_t<uint32_t> counts(static_cast<py::ssize_t>(nq));
    uint32_t *cp = counts.mutable_data();
    float *dp = dists.mutable_data();
    last_counters_.assign(nq * 4, 0);
    if (radius_mode) {
      // more_append: a later chunk of one Index.range_search call, whose rows go behind the earlier chunks'
      const size_t at = more_append ? last_range_more_.size() : 0;
      last_range_more_.resize(at);
      last_range_more_.resize(at + nq * 2, 0);
      uint32_t *mp = last_range_more_.data() + at;
      py::gil_scoped_release nogil;
      check(alaya_index_range_search_radius(ix_, static_cast<const float *>(q.data()), nq, ef, radii.data(), max_results,
                                            m.words, m.n_masks, m.of_query, cp, ids32.data(), dp, last_counters_.data(),
                                            max_frontier, mp));
    } else {
      py::gil_scoped_release nogil;
      check(alaya_index_range_search(ix_, static_cast<const float *>(q.data()), nq, ef, radii.data(), max_results, m.words,
                                     m.n_masks, m.of_query, cp, ids32.data(), dp, last_counters_.data()));
    }
    return py::make_tuple(counts, widen_ids(ids32, nq, max_results, true), dists, last_counters());
  }

  // --- extra (not in the reference binding): range_search on an SQ8 index (alaya_index_range_search_sq8).  The
  // traversal of batch_search at `ef` runs on the codes; the valid, allowed rows it measures within `code_radius`
  // by code distance are candidates, the first max_results of them are measured exactly and those within `radius`
  // are the hits.  Returns range_search's tuple with counts the hits; last_range_candidates() holds the candidate
  // counts (cand_append: behind an earlier chunk's of one Index.range_search call).  The query forms are
  // filtered_search's on an SQ8 index.
  py::object range_search_sq8(py::array queries, uint32_t ef, py::object radius, py::object code_radius,
                              uint32_t max_results, py::object allow_words, py::object mask_of_query, bool cand_append) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    if (params_.quantization_type_ != QuantizationType::SQ8)
      throw py::value_error("range_search_sq8 searches SQ8 indexes only");
    py::array q = prepare_queries(queries);
    const uint64_t nq = q.shape(0);
    U32Array words;
    const Masks m = parse_range_masks(allow_words, words, mask_of_query, n_, nq);
    const std::vector<float> radii = parse_radii(radius, nq);
    const std::vector<float> code_radii = parse_radii(code_radius, nq);
    if (max_results == 0 || max_results > 4096) throw py::value_error("max_results must be in 1..4096");
    std::vector<uint32_t> ids32(nq * max_results);
    py::array_t<float> dists = out2d<float>(nq, max_results);
    py::array_t<uint32_t> counts(static_cast<py::ssize_t>(nq));
    uint32_t *cp = counts.mutable_data();
    float *dp = dists.mutable_data();
    last_counters_.assign(nq * 4, 0);
    std::vector<uint32_t> cand(nq, 0);  // joins last_range_cand_ only once the call has succeeded
    uint32_t *np = cand.data();
    const float *qp = static_cast<const float *>(q.data());
    // the traversal encodes the query as given, the rerank's f32 distance takes the normalised one (run())
    const float *sq = raw_queries_.empty() ? qp : raw_queries_.data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_range_search_sq8(ix_, sq, qp, nq, ef, radii.data(), code_radii.data(), max_results, m.words,
                                         m.n_masks, m.of_query, cp, np, ids32.data(), dp, last_counters_.data()));
    }
    if (!cand_append) last_range_cand_.clear();
    last_range_cand_.insert(last_range_cand_.end(), cand.begin(), cand.end());
    return py::make_tuple(counts, widen_ids(ids32, nq, max_results, true), dists, last_counters());
  }

  uint64_t get_data_num() const { return n_; }

  py::array get_data_by_id(uint32_t id) {
    if (n_ == 0) throw std::runtime_error("space is nullptr");
    if (id >= n_) throw std::runtime_error("id out of range");
    const size_t es = dtype_size(dtype_);
    py::array out(params_.data_type_, std::vector<py::ssize_t>{static_cast<py::ssize_t>(dim_)});
    std::memcpy(out.mutable_data(), raw_.data() + static_cast<size_t>(id) * dim_ * es, dim_ * es);
    return out;
  }

  // PyIndex::insert -> GraphUpdateJob::insert_and_update (index.hpp:229-232,
  // graph_update_job.hpp:65-89): device search_solo for R neighbours, host update job, HBM patch.
  py::object insert(py::array insert_data, uint32_t ef) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    if (params_.quantization_type_ != QuantizationType::NONE)
      throw std::runtime_error("insert on quantized indexes is not supported by the MI355X engine");
    check_dtype(insert_data);
    if (insert_data.ndim() != 1 || static_cast<uint32_t>(insert_data.shape(0)) != dim_)
      throw std::runtime_error("vector dimension mismatch");
    py::array arr = py::array::ensure(insert_data, py::array::c_style);
    ensure_updates();
    // COS: search_solo's QueryComputer normalises the caller's vector in place (raw_space.hpp:
    // 267-269), then RawSpace::insert normalises it again (:146-150).
    std::vector<float> q(dim_), row(dim_);
    if (params_.metric_ == MetricType::COS) normalize_in_place(arr, 1);
    to_float(arr.data(), dtype_, dim_, q.data());
    if (params_.metric_ == MetricType::COS) normalize_in_place(arr, 1);
    to_float(arr.data(), dtype_, dim_, row.data());
    uint64_t id = 0;
    {
      py::gil_scoped_release nogil;
      check(alaya_index_insert(ix_, q.data(), row.data(), ef, &id));
    }
    if (id == kNoId64) return py::int_(id_bytes_ == 4 ? uint64_t{0xffffffffu} : kNoId64);
    const size_t es = dtype_size(dtype_);
    raw_.insert(raw_.end(), static_cast<const char *>(arr.data()), static_cast<const char *>(arr.data()) + dim_ * es);
    rows_f32_.insert(rows_f32_.end(), row.begin(), row.end());
    n_ += 1;
    if (!valid_.empty()) {
      valid_.resize((n_ + 7) / 8, 0);
      valid_[id / 8] |= static_cast<uint8_t>(1u << (id % 8));
    }
    graph_dirty_ = true;
    return py::int_(id);
  }

  // --- extra (not in the reference binding): append rows in bulk by continuing the batched device build
  // (alaya_index_extend_graph) with fit(builder="gpu")'s seed and schedule, whatever built the graph.
  // Rows are checked and, for COS, normalised in place as fit does; an SQ8 index encodes them on the
  // device with its fitted quantizer (values outside the fitted range clamp).  Returns the first new id.
  uint64_t add(py::array vectors, uint32_t ef_construction) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    if (vectors.ndim() != 2) throw std::runtime_error("Array must be 2D");
    check_dtype(vectors);
    if (static_cast<uint32_t>(vectors.shape(1)) != dim_) throw std::runtime_error("vector dimension mismatch");
    py::array arr = py::array::ensure(vectors, py::array::c_style);
    const uint64_t m = arr.shape(0), n0 = n_;
    if (n0 + m > params_.capacity_) throw std::runtime_error("The index is full, cannot insert more vectors");
    if (m == 0) return n0;
    if (params_.metric_ == MetricType::COS) normalize_in_place(arr, m);
    std::vector<float> rows(m * dim_);
    to_float(arr.data(), dtype_, m * dim_, rows.data());
    const bool sq8 = params_.quantization_type_ == QuantizationType::SQ8;
    std::vector<uint8_t> codes(sq8 ? m * dim_ : 0);
    alaya_graph *g = nullptr;
    {
      py::gil_scoped_release nogil;
      uint64_t st[8] = {0};
      check(alaya_index_extend_graph(ix_, rows.data(), m, ef_construction, 100, 0, 0, 2, &g, st));
      last_build_us_ = st[5];
      if (sq8) check(alaya_index_read_sq8(ix_, n0, m, codes.data()));
    }
    alaya_graph_free(graph_);
    graph_ = g;
    graph_dirty_ = false;  // the returned graph is the device's, inserts included; the mirror followed
    const size_t es = dtype_size(dtype_);
    raw_.insert(raw_.end(), static_cast<const char *>(arr.data()), static_cast<const char *>(arr.data()) + m * dim_ * es);
    rows_f32_.insert(rows_f32_.end(), rows.begin(), rows.end());
    sq_codes_.insert(sq_codes_.end(), codes.begin(), codes.end());
    n_ += m;
    if (!valid_.empty()) {
      valid_.resize((n_ + 7) / 8, 0);
      for (uint64_t i = n0; i < n_; ++i) valid_[i / 8] |= static_cast<uint8_t>(1u << (i % 8));
    }
    return n0;
  }

  // the SQ8 codes the device searches, rows [0, n) x dim (tests, tools)
  py::array sq8_codes() {
    if (params_.quantization_type_ != QuantizationType::SQ8) throw std::runtime_error("not an SQ8 index");
    py::array_t<uint8_t> out = out2d<uint8_t>(n_, dim_);
    check(alaya_index_read_sq8(ix_, 0, n_, out.mutable_data()));
    return out;
  }
  // device time of the last fit(builder="gpu") or add: the build steps alone (tools/add_sweep.py)
  double last_build_device_ms() const { return static_cast<double>(last_build_us_) / 1000.0; }
  py::tuple sq8_range() const {
    py::array_t<float> mn(static_cast<py::ssize_t>(sq_min_.size())), mx(static_cast<py::ssize_t>(sq_max_.size()));
    if (!sq_min_.empty()) {
      std::memcpy(mn.mutable_data(), sq_min_.data(), sq_min_.size() * 4);
      std::memcpy(mx.mutable_data(), sq_max_.data(), sq_max_.size() * 4);
    }
    return py::make_tuple(mn, mx);
  }

  // PyIndex::remove -> GraphUpdateJob::remove (index.hpp:234, graph_update_job.hpp:91-103)
  void remove(uint32_t id) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    if (params_.quantization_type_ != QuantizationType::NONE)
      throw std::runtime_error("remove on quantized indexes is not supported by the MI355X engine");
    if (id >= n_) throw std::runtime_error("id out of range");
    ensure_updates();
    check(alaya_index_remove(ix_, id));
    if (valid_.empty()) {
      valid_.assign((n_ + 7) / 8, 0);
      for (uint64_t i = 0; i < n_; ++i) valid_[i / 8] |= static_cast<uint8_t>(1u << (i % 8));
    }
    valid_[id / 8] &= static_cast<uint8_t>(~(1u << (id % 8)));
    delete_cnt_ += 1;  // RawSpace::remove counts every call (raw_space.hpp:160-163)
  }

  // PyIndex::save (index.hpp:113-130): graph file + raw data file (+ quant file)
  void save(const std::string &index_path, const std::string &data_path, const std::string &quant_path) {
    if (!graph_) throw std::runtime_error("index is not fitted");
    sync_graph();
    check(alaya_graph_save(graph_, index_path.c_str(), id_bytes_, std::max<uint64_t>(params_.capacity_, n_),
                           valid_.empty() ? nullptr : valid_.data()));
    if (!data_path.empty()) save_raw(data_path);
    if (!quant_path.empty()) {
      if (params_.quantization_type_ != QuantizationType::SQ8) throw std::runtime_error("no quantized space to save");
      save_sq8(quant_path);
    }
  }

  void load(const std::string &index_path, const std::string &data_path, const std::string &quant_path) {
    if (graph_) alaya_graph_free(graph_);
    graph_ = nullptr;
    check(alaya_graph_load(index_path.c_str(), id_bytes_, &graph_));
    if (data_path.empty()) throw std::runtime_error("the MI355X engine needs the raw data file");
    load_raw(data_path);
    if (params_.quantization_type_ == QuantizationType::SQ8) {
      if (quant_path.empty()) throw std::runtime_error("SQ8 index needs its quant file");
      load_sq8(quant_path);
    }
    upload();
  }

  uint32_t get_data_dim() const { return dim_; }

  // --- extra (not in the reference binding): device counters of the last search ---
  // rows stepped through per query of the last filtered_search(..., through=True); empty after any other
  // candidates per query of the last range_search_sq8: shape (nq,)
  py::array last_range_candidates() const {
    py::array_t<uint32_t> out(static_cast<py::ssize_t>(last_range_cand_.size()));
    if (!last_range_cand_.empty()) std::memcpy(out.mutable_data(), last_range_cand_.data(), last_range_cand_.size() * 4);
    return out;
  }
  // (frontier, more_dist) per query of the last radius-mode range_search: shape (nq, 2)
  py::array last_range_more() const {
    py::array_t<uint32_t> out = out2d<uint32_t>(last_range_more_.size() / 2, 2);
    if (!last_range_more_.empty()) std::memcpy(out.mutable_data(), last_range_more_.data(), last_range_more_.size() * 4);
    return out;
  }
  py::array last_through() const {
    py::array_t<uint32_t> out(static_cast<py::ssize_t>(last_through_.size()));
    if (!last_through_.empty()) std::memcpy(out.mutable_data(), last_through_.data(), last_through_.size() * 4);
    return out;
  }
  py::array last_counters() const {
    py::array_t<uint32_t> out = out2d<uint32_t>(last_counters_.size() / 4, 4);
    std::memcpy(out.mutable_data(), last_counters_.data(), last_counters_.size() * 4);
    return out;
  }
  // SQ8 batch_search rerank: 1 = the reference's PyIndex::rerank (default), 2 = corrected (whole ef pool)
  void set_rerank_mode(int m) {
    if (m != 1 && m != 2) throw std::invalid_argument("rerank mode must be 1 (reference) or 2 (corrected)");
    rerank_mode_ = m;
  }
  int rerank_mode() const { return rerank_mode_; }
  py::array device_distances(py::array queries, py::array_t<uint32_t> ids) {
    py::array q = prepare_queries(queries);
    U32Array idc(ids);
    const uint64_t nq = q.shape(0);
    const uint32_t n = static_cast<uint32_t>(idc.size());
    py::array_t<float> out = out2d<float>(nq, n);
    check(alaya_index_distances(ix_, static_cast<const float *>(q.data()), nq, idc.data(), n,
                                out.mutable_data()));
    return out;
  }
  // graph arrays (n x R l0, levels, upper_off, upper_edges, ep, upper_R) for tests/tools
  py::tuple graph_arrays() {
    if (!graph_) throw std::runtime_error("index is not fitted");
    sync_graph();
    return graph_arrays_of(graph_);
  }

 private:
  int metric_code() const {
    switch (params_.metric_) {
      case MetricType::L2: return ALAYA_METRIC_L2;
      case MetricType::IP: return ALAYA_METRIC_IP;
      case MetricType::COS: return ALAYA_METRIC_COS;
      default: throw std::runtime_error("unsupported metric");
    }
  }

  // the metric plus ALAYA_DIST_GENERIC for non-float DataType: l2_sqr<T>/ip_sqr<T> take their generic
  // branch for every DataType but float (distance_l2.ipp:735-741, distance_ip.ipp:744-750)
  int dist_code() const { return metric_code() | (dtype_ != kF32 ? ALAYA_DIST_GENERIC : 0); }

  void check_dtype(const py::array &a) const {
    if (dtype_code(a.dtype()) != dtype_) throw std::runtime_error("Unsupported data type");
  }

  void normalize_in_place(py::array &arr, uint64_t rows) {
    if (!arr.writeable()) throw std::runtime_error("COS metric normalises the input in place; array is read-only");
    if (dtype_ == kF32) {
      float *p = static_cast<float *>(arr.mutable_data());
      for (uint64_t i = 0; i < rows; ++i) alaya_amd::normalize_row(p + i * dim_, dim_);
    } else {  // float64 rows (data_utils.hpp normalize<double>)
      double *p = static_cast<double *>(arr.mutable_data());
      for (uint64_t i = 0; i < rows; ++i) {
        float sum = 0.0f;
        for (uint32_t j = 0; j < dim_; ++j) sum += static_cast<float>(p[i * dim_ + j] * p[i * dim_ + j]);
        sum = static_cast<float>(1.0 / std::sqrt(static_cast<double>(sum)));
        for (uint32_t j = 0; j < dim_; ++j) p[i * dim_ + j] *= sum;
      }
    }
  }

  py::array prepare_queries(py::array queries) {
    if (queries.ndim() != 2) throw std::runtime_error("queries must be 2D");
    check_dtype(queries);
    if (static_cast<uint32_t>(queries.shape(1)) != dim_) throw py::value_error("query dimension mismatch");
    py::array arr = py::array::ensure(queries, py::array::c_style);
    const uint64_t nq = arr.shape(0);
    raw_queries_.clear();
    if (params_.quantization_type_ == QuantizationType::SQ8 && params_.metric_ == MetricType::COS) {
      raw_queries_.resize(nq * dim_);
      to_float(arr.data(), dtype_, nq * dim_, raw_queries_.data());
    }
    if (params_.metric_ == MetricType::COS) normalize_in_place(arr, nq);  // raw_space.hpp:267-269
    py::array_t<float> qf = out2d<float>(nq, dim_);
    to_float(arr.data(), dtype_, nq * dim_, qf.mutable_data());
    return qf;
  }

  std::pair<py::array, py::array> run(py::array queries, uint32_t topk, uint32_t ef, bool want_dist) {
    if (!graph_) throw std::runtime_error("Index is not init yet");
    py::array q = prepare_queries(queries);
    const uint64_t nq = q.shape(0);
    std::vector<uint32_t> ids32(nq * topk);
    py::array_t<float> dists = out2d<float>(nq, topk);
    last_counters_.assign(nq * 4, 0);
    if (params_.quantization_type_ == QuantizationType::SQ8) {
      // SQ8Space::QueryComputer encodes the query as given (no COS normalisation), the rerank's
      // RawSpace::QueryComputer normalises it (raw_space.hpp:267-269): keep both forms.
      const float *rq = static_cast<const float *>(q.data());
      const float *sq = raw_queries_.empty() ? rq : raw_queries_.data();
      // batch_search reranks (index.hpp:337-345); batch_search_with_distance does not and returns
      // an empty distance array for SQ spaces (index.hpp:391-418, get_topk_array of no rows).
      const int rerank = want_dist ? 0 : rerank_mode_;
      {
        py::gil_scoped_release nogil;
        check(alaya_index_batch_search_sq8(ix_, sq, rq, nq, topk, ef, rerank, ids32.data(),
                                           dists.mutable_data(), last_counters_.data()));
      }
      if (want_dist) dists = py::array_t<float>(std::vector<py::ssize_t>{0, static_cast<py::ssize_t>(topk)});
    } else {
      py::gil_scoped_release nogil;
      check(alaya_index_batch_search(ix_, static_cast<const float *>(q.data()), nq, topk, ef,
                                     ids32.data(), dists.mutable_data(), last_counters_.data()));
    }
    // no empty id to map here: batch_search fills short results with id 0, as the reference does
    return {widen_ids(ids32, nq, topk, false), want_dist ? py::array(dists) : py::array()};
  }

  // The device's 32-bit ids in the index's id type.  map_empty: the empty slot 0xffffffff becomes the 64-bit
  // type's maximum (the filtered and exact calls; a 32-bit id type holds it as it is).
  py::array widen_ids(const std::vector<uint32_t> &ids32, uint64_t nq, uint32_t topk, bool map_empty) const {
    py::array ids(params_.id_type_, std::vector<py::ssize_t>{static_cast<py::ssize_t>(nq), static_cast<py::ssize_t>(topk)});
    if (id_bytes_ == 4) {
      std::memcpy(ids.mutable_data(), ids32.data(), ids32.size() * 4);
    } else {
      auto *o = static_cast<uint64_t *>(ids.mutable_data());
      for (size_t i = 0; i < ids32.size(); ++i) o[i] = map_empty && ids32[i] == 0xffffffffu ? kNoId64 : ids32[i];
    }
    return ids;
  }

  // first insert/remove: hand the device index a host mirror of the graph, rows and bitmap
  void ensure_updates() {
    if (updates_enabled_) return;
    const uint64_t cap = std::max<uint64_t>(params_.capacity_, n_);
    check(alaya_index_enable_updates(ix_, graph_, rows_f32_.data(), n_, cap, valid_.empty() ? nullptr : valid_.data()));
    updates_enabled_ = true;
  }
  // replace the (stale) fitted graph with the updated mirror
  void sync_graph() {
    if (!graph_dirty_) return;
    alaya_graph *g = nullptr;
    check(alaya_index_export_graph(ix_, &g));
    alaya_graph_free(graph_);
    graph_ = g;
    graph_dirty_ = false;
  }

  void upload() {
    updates_enabled_ = false;
    graph_dirty_ = false;
    if (!graph_) return;
    uint64_t gn = 0;
    check(alaya_graph_info(graph_, &gn, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    py::gil_scoped_release nogil;
    check(alaya_index_set_base(ix_, rows_f32_.data(), n_, dim_, dist_code(),
                               valid_.empty() ? nullptr : valid_.data()));
    check(alaya_index_set_graph(ix_, graph_));
    if (!sq_codes_.empty())
      check(alaya_index_set_sq8(ix_, sq_codes_.data(), n_, dim_, sq_min_.data(), sq_max_.data(), host_sq8_order()));
  }

  void train_sq8(uint32_t num_threads) {
    if (params_.metric_ == MetricType::COS && dtype_ != kF32) throw std::runtime_error("COS metric only support float or double");
    sq_min_.assign(dim_, 0.f);
    sq_max_.assign(dim_, 0.f);
    sq_codes_.assign(n_ * dim_, 0);
    check(alaya_sq8_train(rows_f32_.data(), n_, dim_, sq_min_.data(), sq_max_.data()));
    check(alaya_sq8_encode(rows_f32_.data(), n_, dim_, sq_min_.data(), sq_max_.data(), sq_codes_.data(),
                           std::max(1u, num_threads)));
  }

  // RawSpace save/load (raw_space.hpp:219-250) + SequentialStorage (sequential_storage.hpp:110-142)
  // What the raw and the SQ8 space files share: the space header, then SequentialStorage's -- its header, the
  // capacity's rows of `item` bytes each padded to 64, the validity bitmap (valid empty = every row).
  void write_space(std::ofstream &w, uint32_t item, uint64_t delete_cnt, const void *rows,
                   const std::vector<uint8_t> &valid) const {
    const int32_t metric = static_cast<int32_t>(params_.metric_);
    const uint64_t cap = std::max<uint64_t>(params_.capacity_, n_);
    w.write(reinterpret_cast<const char *>(&metric), 4);
    w.write(reinterpret_cast<const char *>(&item), 4);  // data_size_
    w.write(reinterpret_cast<const char *>(&dim_), 4);
    for (uint64_t v : {n_, delete_cnt, cap}) {  // item_cnt_, delete_cnt_, capacity_ in the id type
      const uint32_t x = static_cast<uint32_t>(v);
      if (id_bytes_ == 4) w.write(reinterpret_cast<const char *>(&x), 4);
      else w.write(reinterpret_cast<const char *>(&v), 8);
    }
    const uint64_t hdr[5] = {item, (item + 63ull) / 64 * 64, cap, n_, 64};  // item, aligned item, capacity, pos, alignment
    w.write(reinterpret_cast<const char *>(hdr), sizeof(hdr));
    std::vector<char> row(hdr[1], 0);
    for (uint64_t i = 0; i < cap; ++i) {
      std::fill(row.begin(), row.end(), 0);
      if (i < n_) std::memcpy(row.data(), static_cast<const char *>(rows) + i * item, item);
      w.write(row.data(), static_cast<std::streamsize>(row.size()));
    }
    std::vector<uint8_t> bitmap((cap + 7) / 8, 0);
    for (uint64_t i = 0; i < n_; ++i)
      if (valid.empty() || (valid[i / 8] >> (i % 8)) & 1) bitmap[i / 8] |= static_cast<uint8_t>(1u << (i % 8));
    w.write(reinterpret_cast<const char *>(bitmap.data()), static_cast<std::streamsize>(bitmap.size()));
  }

  void save_raw(const std::string &path) const {
    std::ofstream w(path, std::ios::binary);
    if (!w.is_open()) throw std::runtime_error("Cannot open file " + path);
    write_space(w, static_cast<uint32_t>(dim_ * dtype_size(dtype_)), delete_cnt_, raw_.data(), valid_);
    if (!w) throw std::runtime_error("write failed: " + path);
  }

  void load_raw(const std::string &path) {
    std::ifstream r(path, std::ios::binary);
    if (!r.is_open()) throw std::runtime_error("Cannot open file " + path);
    int32_t metric;
    uint32_t data_size, dim;
    r.read(reinterpret_cast<char *>(&metric), 4);
    r.read(reinterpret_cast<char *>(&data_size), 4);
    r.read(reinterpret_cast<char *>(&dim), 4);
    auto get_id = [&]() -> uint64_t {
      if (id_bytes_ == 4) {
        uint32_t x;
        r.read(reinterpret_cast<char *>(&x), 4);
        return x;
      }
      uint64_t x;
      r.read(reinterpret_cast<char *>(&x), 8);
      return x;
    };
    const uint64_t item_cnt = get_id();
    delete_cnt_ = get_id();
    (void)get_id();
    uint64_t hdr[5];
    r.read(reinterpret_cast<char *>(hdr), sizeof(hdr));
    if (!r) throw std::runtime_error("truncated raw data file");
    const uint64_t item = hdr[0], aligned = hdr[1], cap = hdr[2], pos = hdr[3];
    const size_t es = dtype_size(dtype_);
    if (item != static_cast<uint64_t>(dim) * es || data_size != item || aligned < item)
      throw std::runtime_error("raw data file does not match the index data type");
    dim_ = dim;
    n_ = item_cnt;
    if (pos < n_) n_ = pos;
    raw_.assign(n_ * item, 0);
    std::vector<char> row(aligned);
    for (uint64_t i = 0; i < cap; ++i) {
      r.read(row.data(), static_cast<std::streamsize>(aligned));
      if (!r) throw std::runtime_error("truncated raw data file");
      if (i < n_) std::memcpy(raw_.data() + i * item, row.data(), item);
    }
    std::vector<uint8_t> bitmap((cap + 7) / 8);
    r.read(reinterpret_cast<char *>(bitmap.data()), static_cast<std::streamsize>(bitmap.size()));
    valid_.assign((n_ + 7) / 8, 0);
    bool all = true;
    for (uint64_t i = 0; i < n_; ++i) {
      const bool v = (bitmap[i / 8] >> (i % 8)) & 1;
      if (v) valid_[i / 8] |= static_cast<uint8_t>(1u << (i % 8)); else all = false;
    }
    if (all) valid_.clear();
    rows_f32_.resize(n_ * dim_);
    to_float(raw_.data(), dtype_, n_ * dim_, rows_f32_.data());
  }

  // SQ8Space save/load (sq8_space.hpp:213-251) + SQ8Quantizer (sq8.hpp:161-177)
  void save_sq8(const std::string &path) const {
    std::ofstream w(path, std::ios::binary);
    if (!w.is_open()) throw std::runtime_error("Cannot open file " + path);
    write_space(w, dim_, 0, sq_codes_.data(), {});  // one byte per dimension, no delete count, every row valid
    w.write(reinterpret_cast<const char *>(&dim_), 4);
    w.write(reinterpret_cast<const char *>(sq_min_.data()), dim_ * 4);
    w.write(reinterpret_cast<const char *>(sq_max_.data()), dim_ * 4);
    if (!w) throw std::runtime_error("write failed: " + path);
  }
  void load_sq8(const std::string &path) {
    std::ifstream r(path, std::ios::binary);
    if (!r.is_open()) throw std::runtime_error("Cannot open file " + path);
    int32_t metric;
    uint32_t data_size, dim;
    r.read(reinterpret_cast<char *>(&metric), 4);
    r.read(reinterpret_cast<char *>(&data_size), 4);
    r.read(reinterpret_cast<char *>(&dim), 4);
    r.ignore(3 * id_bytes_);
    uint64_t hdr[5];
    r.read(reinterpret_cast<char *>(hdr), sizeof(hdr));
    if (!r || dim != dim_ || hdr[0] != dim) throw std::runtime_error("SQ8 file does not match the raw data");
    const uint64_t aligned = hdr[1], cap = hdr[2];
    sq_codes_.assign(n_ * dim_, 0);
    std::vector<char> row(aligned);
    for (uint64_t i = 0; i < cap; ++i) {
      r.read(row.data(), static_cast<std::streamsize>(aligned));
      if (!r) throw std::runtime_error("truncated SQ8 file");
      if (i < n_) std::memcpy(sq_codes_.data() + i * dim_, row.data(), dim_);
    }
    r.ignore(static_cast<std::streamsize>((cap + 7) / 8));
    uint32_t qd = 0;
    r.read(reinterpret_cast<char *>(&qd), 4);
    if (qd != dim_) throw std::runtime_error("SQ8 quantizer dimension mismatch");
    sq_min_.resize(dim_);
    sq_max_.resize(dim_);
    r.read(reinterpret_cast<char *>(sq_min_.data()), dim_ * 4);
    r.read(reinterpret_cast<char *>(sq_max_.data()), dim_ * 4);
    if (!r) throw std::runtime_error("truncated SQ8 file");
  }

  IndexParams params_;
  DType dtype_ = kF32;
  int id_bytes_ = 4;
  alaya_graph *graph_ = nullptr;
  uint64_t n_ = 0;
  uint32_t dim_ = 0;
  std::vector<char> raw_;          // original-dtype rows (get_data_by_id, save)
  std::vector<float> rows_f32_;    // float rows uploaded to HBM
  std::vector<uint8_t> valid_;     // empty = all valid
  uint64_t delete_cnt_ = 0;        // RawSpace::delete_cnt_
  uint64_t last_build_us_ = 0;     // last_build_device_ms
  bool updates_enabled_ = false;   // the device index holds an update mirror (alaya_index_enable_updates)
  bool graph_dirty_ = false;       // graph_ predates inserts (sync_graph refreshes it)
  std::vector<uint32_t> last_counters_;
  std::vector<uint32_t> last_through_;
  std::vector<uint32_t> last_range_more_;
  std::vector<uint32_t> last_range_cand_;  // candidate counts of the last range_search_sq8 (chunks concatenated)
  int rerank_mode_ = 1;
  std::vector<float> raw_queries_;   // SQ8 + COS: the un-normalised queries the SQ8 search encodes
  std::vector<uint8_t> sq_codes_;
  std::vector<float> sq_min_, sq_max_;
};


// ---- engine-level objects (beyond the reference binding): host graph + raw device index -----
class Graph {
 public:
  Graph() = default;
  explicit Graph(alaya_graph *g) : g_(g) {}
  ~Graph() {
    if (g_) alaya_graph_free(g_);
  }
  Graph(const Graph &) = delete;
  Graph &operator=(const Graph &) = delete;

  static std::shared_ptr<Graph> build(F32Array data, int metric, uint32_t R, uint32_t efc, uint32_t threads,
                                      uint64_t seed) {
    if (data.ndim() != 2) throw py::value_error("data must be 2D");
    alaya_graph *g = nullptr;
    const float *ptr = data.data();
    const uint64_t n = data.shape(0);
    const uint32_t d = static_cast<uint32_t>(data.shape(1));
    {
      py::gil_scoped_release nogil;
      check(alaya_graph_build_hnsw(ptr, n, d, metric, R, efc, threads, seed, &g));
    }
    return std::make_shared<Graph>(g);
  }
  static std::shared_ptr<Graph> load(const std::string &path, int id_bytes) {
    alaya_graph *g = nullptr;
    check(alaya_graph_load(path.c_str(), id_bytes, &g));
    return std::make_shared<Graph>(g);
  }
  static std::shared_ptr<Graph> from_arrays(U32Array l0, py::object levels, py::object upper_off, py::object upper_edges,
                                            uint32_t upper_R, uint32_t ep, py::object eps) {
    alaya_graph *g = nullptr;
    const uint64_t n = l0.shape(0);
    const uint32_t R = static_cast<uint32_t>(l0.shape(1));
    if (!levels.is_none()) {
      auto lv = U32Array(levels);
      auto off = CArray<uint64_t>(upper_off);
      auto ue = U32Array(upper_edges);
      check(alaya_graph_import(n, R, l0.data(), lv.data(), off.data(), ue.data(), ue.size(), upper_R, ep,
                               nullptr, 0, &g));
    } else {
      auto e = U32Array(eps);
      check(alaya_graph_import(n, R, l0.data(), nullptr, nullptr, nullptr, 0, 0, 0, e.data(),
                               static_cast<uint32_t>(e.size()), &g));
    }
    return std::make_shared<Graph>(g);
  }
  void save(const std::string &path, int id_bytes, uint64_t capacity) const {
    check(alaya_graph_save(g_, path.c_str(), id_bytes, capacity, nullptr));
  }
  py::tuple arrays() const { return graph_arrays_of(g_); }
  alaya_graph *get() const { return g_; }

 private:
  alaya_graph *g_ = nullptr;
};

// Raw device index: rows + graph in HBM, batch search on host arrays or device pointers.
class DeviceIndex : public LaunchControls {
 public:
  explicit DeviceIndex(int device) { check(alaya_index_create(device, &ix_)); }
  ~DeviceIndex() {
    if (ix_) alaya_index_destroy(ix_);
  }
  DeviceIndex(const DeviceIndex &) = delete;
  DeviceIndex &operator=(const DeviceIndex &) = delete;
  void set_base(F32Array rows, int metric, py::object valid) {
    const uint8_t *vp = nullptr;
    U8Array v;
    if (!valid.is_none()) {
      v = U8Array(valid);
      vp = v.data();
    }
    const float *ptr = rows.data();
    const uint64_t n = rows.shape(0);
    const uint32_t d = static_cast<uint32_t>(rows.shape(1));
    py::gil_scoped_release nogil;
    check(alaya_index_set_base(ix_, ptr, n, d, metric, vp));
  }
  void set_graph(const Graph &g) { check(alaya_index_set_graph(ix_, g.get())); }
  // device HNSW build from the rows set by set_base; the graph becomes this index's search graph
  py::tuple build_graph(uint32_t R, uint32_t efc, uint64_t seed, uint32_t batch_div, uint32_t max_batch,
                        uint32_t refine) {
    alaya_graph *g = nullptr;
    uint64_t st[8] = {0};
    {
      py::gil_scoped_release nogil;
      check(alaya_index_build_graph(ix_, R, efc, seed, batch_div, max_batch, refine, &g, st));
    }
    return py::make_tuple(std::make_shared<Graph>(g), build_stats(st));
  }
  // append rows by continuing the device build on the installed graph (alaya_index_extend_graph): the
  // whole grown graph and the stats of this call's batches
  py::tuple extend_graph(F32Array rows, uint32_t efc, uint64_t seed, uint32_t batch_div, uint32_t max_batch,
                         uint32_t refine) {
    uint64_t n = 0;
    uint32_t dim = 0;
    check(alaya_index_info(ix_, &n, &dim, nullptr, nullptr, nullptr));
    if (rows.ndim() != 2 || static_cast<uint32_t>(rows.shape(1)) != dim)
      throw py::value_error("rows must be 2D with the index's width");
    alaya_graph *g = nullptr;
    uint64_t st[8] = {0};
    const float *ptr = rows.data();
    const uint64_t count = rows.shape(0);
    {
      py::gil_scoped_release nogil;
      check(alaya_index_extend_graph(ix_, ptr, count, efc, seed, batch_div, max_batch, refine, &g, st));
    }
    return py::make_tuple(std::make_shared<Graph>(g), build_stats(st));
  }
  py::array read_sq8(uint64_t first, uint64_t count) {
    uint32_t dim = 0;
    check(alaya_index_info(ix_, nullptr, &dim, nullptr, nullptr, nullptr));
    py::array_t<uint8_t> out = out2d<uint8_t>(count, dim);
    check(alaya_index_read_sq8(ix_, first, count, out.mutable_data()));
    return out;
  }
  static py::dict build_stats(const uint64_t *st) {
    py::dict stats;
    stats["batches"] = st[0];
    stats["launches"] = st[1];
    stats["prunes"] = st[2];
    stats["appends"] = st[3];
    stats["heuristic_dists"] = st[4];
    stats["device_ms"] = static_cast<double>(st[5]) / 1000.0;
    stats["max_batch"] = st[6];
    stats["max_level"] = st[7];
    return stats;
  }
  py::tuple search(F32Array q, uint32_t k, uint32_t ef) {
    const uint64_t nq = q.shape(0);
    Results r(nq, k);
    const float *qp = q.data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_batch_search(ix_, qp, nq, k, ef, r.ip, r.dp, r.cp));
    }
    return py::make_tuple(r.ids, r.d, r.c);
  }
  void search_device(uintptr_t q, uint64_t nq, uint32_t k, uint32_t ef, uintptr_t ids, uintptr_t dists,
                     uintptr_t counters, uintptr_t stream) {
    check(alaya_index_batch_search_device(ix_, dptr<const float>(q), nq, k, ef, dptr<uint32_t>(ids), dptr<float>(dists),
                                          dptr<uint32_t>(counters), dptr<void>(stream)));
  }
  // the k nearest rows among those allow_words (uint32 [n_masks, ceil(n / 32)], utils.pack_allow) allows;
  // mask_of_query: each query's mask, or None with one mask
  py::tuple filtered_search(F32Array q, uint32_t k, uint32_t ef, U32Array allow_words, py::object mask_of_query) {
    return filtered_search_call(q, k, ef, allow_words, mask_of_query, false);
  }
  // the same under the traversal that steps through disallowed neighbours (alaya_index_filtered_search_hop):
  // (ids, dists, counters[nq, 4], n_through[nq])
  py::tuple filtered_search_hop(F32Array q, uint32_t k, uint32_t ef, U32Array allow_words, py::object mask_of_query) {
    return filtered_search_call(q, k, ef, allow_words, mask_of_query, true);
  }
  py::tuple filtered_search_call(F32Array q, uint32_t k, uint32_t ef, U32Array allow_words, py::object mask_of_query,
                                 bool hop) {
    const uint64_t nq = q.shape(0);
    const Masks m = parse_masks(allow_words, mask_of_query, rows(), nq);
    Results r(nq, k);
    const float *qp = q.data();
    if (hop) {
      py::array_t<uint32_t> t(static_cast<py::ssize_t>(nq));
      uint32_t *tp = t.mutable_data();
      {
        py::gil_scoped_release nogil;
        check(alaya_index_filtered_search_hop(ix_, qp, nq, k, ef, m.words, m.n_masks, m.of_query, r.ip, r.dp, r.cp, tp));
      }
      return py::make_tuple(r.ids, r.d, r.c, t);
    }
    {
      py::gil_scoped_release nogil;
      check(alaya_index_filtered_search(ix_, qp, nq, k, ef, m.words, m.n_masks, m.of_query, r.ip, r.dp, r.cp));
    }
    return py::make_tuple(r.ids, r.d, r.c);
  }
  void filtered_search_hop_device(uintptr_t q, uint64_t nq, uint32_t k, uint32_t ef, uintptr_t allow_words, uint32_t n_masks,
                                  uintptr_t mask_of_query, uintptr_t ids, uintptr_t dists, uintptr_t counters,
                                  uintptr_t n_through, uintptr_t stream) {
    check(alaya_index_filtered_search_hop_device(ix_, dptr<const float>(q), nq, k, ef, dptr<const uint32_t>(allow_words),
                                                 n_masks, dptr<const uint32_t>(mask_of_query), dptr<uint32_t>(ids),
                                                 dptr<float>(dists), dptr<uint32_t>(counters), dptr<uint32_t>(n_through),
                                                 dptr<void>(stream)));
  }
  void filtered_search_device(uintptr_t q, uint64_t nq, uint32_t k, uint32_t ef, uintptr_t allow_words, uint32_t n_masks,
                              uintptr_t mask_of_query, uintptr_t ids, uintptr_t dists, uintptr_t counters,
                              uintptr_t stream) {
    check(alaya_index_filtered_search_device(ix_, dptr<const float>(q), nq, k, ef, dptr<const uint32_t>(allow_words),
                                             n_masks, dptr<const uint32_t>(mask_of_query), dptr<uint32_t>(ids),
                                             dptr<float>(dists), dptr<uint32_t>(counters), dptr<void>(stream)));
  }
  // every row the traversal measures within `radius` (a number or one per query) of the query
  // (alaya_index_range_search): (counts[nq], ids[nq, max_results], dists[nq, max_results], counters[nq, 4]);
  // allow_words / mask_of_query as for filtered_search, or None for no mask
  py::tuple range_search(F32Array q, uint32_t ef, py::object radius, uint32_t max_results, py::object allow_words,
                         py::object mask_of_query) {
    const uint64_t nq = q.shape(0);
    U32Array words;
    const Masks m = parse_range_masks(allow_words, words, mask_of_query, rows(), nq);
    const std::vector<float> radii = parse_radii(radius, nq);
    if (max_results == 0 || max_results > 4096) throw py::value_error("max_results must be in 1..4096");
    Results r(nq, max_results);
    py::array_t<uint32_t> counts(static_cast<py::ssize_t>(nq));
    uint32_t *np = counts.mutable_data();
    const float *qp = q.data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_range_search(ix_, qp, nq, ef, radii.data(), max_results, m.words, m.n_masks, m.of_query, np, r.ip,
                                     r.dp, r.cp));
    }
    return py::make_tuple(counts, r.ids, r.d, r.c);
  }
  // the radius mode (alaya_index_range_search_radius): the same and more[nq, 2] = (frontier, more_dist)
  py::tuple range_search_radius(F32Array q, uint32_t ef, py::object radius, uint32_t max_results, uint32_t max_frontier,
                                py::object allow_words, py::object mask_of_query) {
    const uint64_t nq = q.shape(0);
    U32Array words;
    const Masks m = parse_range_masks(allow_words, words, mask_of_query, rows(), nq);
    const std::vector<float> radii = parse_radii(radius, nq);
    if (max_results == 0 || max_results > 4096) throw py::value_error("max_results must be in 1..4096");
    if (max_frontier == 0 || max_frontier > 16384) throw py::value_error("max_frontier must be in 1..16384");
    Results r(nq, max_results);
    py::array_t<uint32_t> counts(static_cast<py::ssize_t>(nq));
    py::array_t<uint32_t> more = out2d<uint32_t>(nq, 2);
    uint32_t *np = counts.mutable_data();
    uint32_t *mp = more.mutable_data();
    const float *qp = q.data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_range_search_radius(ix_, qp, nq, ef, radii.data(), max_results, m.words, m.n_masks, m.of_query, np,
                                            r.ip, r.dp, r.cp, max_frontier, mp));
    }
    return py::make_tuple(counts, r.ids, r.d, r.c, more);
  }
  void range_search_radius_device(uintptr_t q, uint64_t nq, uint32_t ef, uintptr_t radii, uint32_t max_results,
                                  uintptr_t allow_words, uint32_t n_masks, uintptr_t mask_of_query, uintptr_t counts,
                                  uintptr_t ids, uintptr_t dists, uintptr_t counters, uintptr_t stream, uint32_t max_frontier,
                                  uintptr_t more) {
    check(alaya_index_range_search_radius_device(ix_, dptr<const float>(q), nq, ef, dptr<const float>(radii), max_results,
                                                 dptr<const uint32_t>(allow_words), n_masks,
                                                 dptr<const uint32_t>(mask_of_query), dptr<uint32_t>(counts),
                                                 dptr<uint32_t>(ids), dptr<float>(dists), dptr<uint32_t>(counters),
                                                 dptr<void>(stream), max_frontier, dptr<uint32_t>(more)));
  }
  void range_search_device(uintptr_t q, uint64_t nq, uint32_t ef, uintptr_t radii, uint32_t max_results,
                           uintptr_t allow_words, uint32_t n_masks, uintptr_t mask_of_query, uintptr_t counts, uintptr_t ids,
                           uintptr_t dists, uintptr_t counters, uintptr_t stream) {
    check(alaya_index_range_search_device(ix_, dptr<const float>(q), nq, ef, dptr<const float>(radii), max_results,
                                          dptr<const uint32_t>(allow_words), n_masks, dptr<const uint32_t>(mask_of_query),
                                          dptr<uint32_t>(counts), dptr<uint32_t>(ids), dptr<float>(dists),
                                          dptr<uint32_t>(counters), dptr<void>(stream)));
  }
  // range search of the index's SQ8 codes, the stored candidates measured on the f32 rows
  // (alaya_index_range_search_sq8): (counts[nq] = hits, ids[nq, max_results], dists[nq, max_results], counters[nq, 4],
  // cand[nq] = candidates within code_radius, not capped); radius / code_radius: a number or one per query;
  // allow_words / groups as range_search's masks; rerank_queries: None = queries
  py::tuple range_search_sq8(F32Array q, uint32_t ef, py::object radius, py::object code_radius, uint32_t max_results,
                             py::object allow_words, py::object mask_of_query, py::object rerank_queries) {
    const uint64_t nq = q.shape(0);
    U32Array words;
    const Masks m = parse_range_masks(allow_words, words, mask_of_query, rows(), nq);
    const std::vector<float> radii = parse_radii(radius, nq);
    const std::vector<float> code_radii = parse_radii(code_radius, nq);
    if (max_results == 0 || max_results > 4096) throw py::value_error("max_results must be in 1..4096");
    F32Array rq;
    const float *rqp = nullptr;
    if (!rerank_queries.is_none()) {
      rq = F32Array(rerank_queries);
      if (rq.ndim() != 2 || rq.shape(0) != q.shape(0) || rq.shape(1) != q.shape(1))
        throw py::value_error("rerank_queries must have the queries' shape");
      rqp = rq.data();
    }
    Results r(nq, max_results);
    py::array_t<uint32_t> counts(static_cast<py::ssize_t>(nq));
    py::array_t<uint32_t> cand(static_cast<py::ssize_t>(nq));
    uint32_t *np = counts.mutable_data();
    uint32_t *cdp = cand.mutable_data();
    const float *qp = q.data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_range_search_sq8(ix_, qp, rqp, nq, ef, radii.data(), code_radii.data(), max_results, m.words,
                                         m.n_masks, m.of_query, np, cdp, r.ip, r.dp, r.cp));
    }
    return py::make_tuple(counts, r.ids, r.d, r.c, cand);
  }
  void range_search_sq8_device(uintptr_t q, uintptr_t rq, uint64_t nq, uint32_t ef, uintptr_t radii, uintptr_t code_radii,
                               uint32_t max_results, uintptr_t allow_words, uint32_t n_masks, uintptr_t mask_of_query,
                               uintptr_t counts, uintptr_t cand, uintptr_t ids, uintptr_t dists, uintptr_t counters,
                               uintptr_t stream) {
    check(alaya_index_range_search_sq8_device(ix_, dptr<const float>(q), dptr<const float>(rq), nq, ef,
                                              dptr<const float>(radii), dptr<const float>(code_radii), max_results,
                                              dptr<const uint32_t>(allow_words), n_masks,
                                              dptr<const uint32_t>(mask_of_query), dptr<uint32_t>(counts),
                                              dptr<uint32_t>(cand), dptr<uint32_t>(ids), dptr<float>(dists),
                                              dptr<uint32_t>(counters), dptr<void>(stream)));
  }
  // the same over the index's SQ8 codes, reranked on the f32 rows (alaya_index_filtered_search_sq8); pool: the
  // candidate pool's capacity, 0 = min(224, max(k, ef)); rerank_queries: None = queries
  py::tuple filtered_search_sq8(F32Array q, uint32_t k, uint32_t ef, U32Array allow_words, py::object mask_of_query,
                                uint32_t pool, py::object rerank_queries) {
    const uint64_t nq = q.shape(0);
    const Masks m = parse_masks(allow_words, mask_of_query, rows(), nq);
    F32Array rq;
    const float *rqp = nullptr;
    if (!rerank_queries.is_none()) {
      rq = F32Array(rerank_queries);
      if (rq.ndim() != 2 || rq.shape(0) != q.shape(0) || rq.shape(1) != q.shape(1))
        throw py::value_error("rerank_queries must have the queries' shape");
      rqp = rq.data();
    }
    Results r(nq, k);
    const float *qp = q.data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_filtered_search_sq8(ix_, qp, rqp, nq, k, ef, pool, m.words, m.n_masks, m.of_query, r.ip, r.dp,
                                            r.cp));
    }
    return py::make_tuple(r.ids, r.d, r.c);
  }
  void filtered_search_sq8_device(uintptr_t q, uintptr_t rq, uint64_t nq, uint32_t k, uint32_t ef, uint32_t pool,
                                  uintptr_t allow_words, uint32_t n_masks, uintptr_t mask_of_query, uintptr_t ids,
                                  uintptr_t dists, uintptr_t counters, uintptr_t stream) {
    check(alaya_index_filtered_search_sq8_device(ix_, dptr<const float>(q), dptr<const float>(rq), nq, k, ef, pool,
                                                 dptr<const uint32_t>(allow_words), n_masks,
                                                 dptr<const uint32_t>(mask_of_query), dptr<uint32_t>(ids),
                                                 dptr<float>(dists), dptr<uint32_t>(counters), dptr<void>(stream)));
  }
  void shard_search_device(uintptr_t q, uint64_t nq, uint32_t k, uint32_t ef, uintptr_t ids, uintptr_t dists,
                           uintptr_t counters, uintptr_t stream) {
    check(alaya_index_shard_search_device(ix_, dptr<const float>(q), nq, k, ef, dptr<uint32_t>(ids), dptr<float>(dists),
                                          dptr<uint32_t>(counters), dptr<void>(stream)));
  }
  py::array distances(F32Array q, U32Array ids) {
    const uint64_t nq = q.shape(0);
    const uint32_t n = static_cast<uint32_t>(ids.size());
    py::array_t<float> out = out2d<float>(nq, n);
    check(alaya_index_distances(ix_, q.data(), nq, ids.data(), n, out.mutable_data()));
    return out;
  }
  void set_sq8(U8Array codes, F32Array mn, F32Array mx, int order) {
    check(alaya_index_set_sq8(ix_, codes.data(), codes.shape(0), static_cast<uint32_t>(codes.shape(1)),
                              mn.data(), mx.data(), order));
  }
  py::tuple search_sq8(F32Array q, uint32_t k, uint32_t ef, int rerank, py::object rerank_queries) {
    const uint64_t nq = q.shape(0);
    F32Array rq;
    const float *rqp = nullptr;
    if (!rerank_queries.is_none()) {
      rq = F32Array(rerank_queries);
      rqp = rq.data();
    }
    Results r(nq, k);
    check(alaya_index_batch_search_sq8(ix_, q.data(), rqp, nq, k, ef, rerank, r.ip, r.dp, r.cp));
    return py::make_tuple(r.ids, r.d, r.c);
  }
  void search_sq8_device(uintptr_t q, uintptr_t rq, uint64_t nq, uint32_t k, uint32_t ef, int rerank,
                         uintptr_t ids, uintptr_t dists, uintptr_t counters, uintptr_t stream) {
    check(alaya_index_batch_search_sq8_device(ix_, dptr<const float>(q), dptr<const float>(rq), nq, k, ef, rerank,
                                              dptr<uint32_t>(ids), dptr<float>(dists), dptr<uint32_t>(counters),
                                              dptr<void>(stream)));
  }
  void shard_search_sq8_device(uintptr_t q, uintptr_t rq, uint64_t nq, uint32_t k, uint32_t ef, bool holds_row0,
                               uintptr_t ids, uintptr_t dists, uintptr_t counters, uintptr_t stream) {
    check(alaya_index_shard_search_sq8_device(ix_, dptr<const float>(q), dptr<const float>(rq), nq, k, ef,
                                              holds_row0 ? 1 : 0, dptr<uint32_t>(ids), dptr<float>(dists),
                                              dptr<uint32_t>(counters), dptr<void>(stream)));
  }
  py::tuple flat_search(F32Array q, uint32_t k) {
    const uint64_t nq = q.shape(0);
    py::array_t<uint32_t> ids = out2d<uint32_t>(nq, k);
    py::array_t<float> d = out2d<float>(nq, k);
    uint32_t redo = 0;
    const float *qp = q.data();
    uint32_t *ip = ids.mutable_data();
    float *dp = d.mutable_data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_flat_search(ix_, qp, nq, k, ip, dp, &redo));
    }
    return py::make_tuple(ids, d, redo);
  }
  void flat_search_device(uintptr_t q, uint64_t nq, uint32_t k, uintptr_t ids, uintptr_t dists,
                          uintptr_t flags, uintptr_t stream) {
    check(alaya_index_flat_search_device(ix_, dptr<const float>(q), nq, k, dptr<uint32_t>(ids), dptr<float>(dists),
                                         dptr<uint32_t>(flags), dptr<void>(stream)));
  }
  // the exact k nearest among the valid rows allow_words (uint32 [n_masks, ceil(n / 32)], utils.pack_allow)
  // allows: a scan of those rows (alaya_index_flat_search_filtered); mask_of_query as for filtered_search
  py::tuple flat_search_filtered(F32Array q, uint32_t k, U32Array allow_words, py::object mask_of_query) {
    const uint64_t nq = q.shape(0);
    const Masks m = parse_masks(allow_words, mask_of_query, rows(), nq);
    py::array_t<uint32_t> ids = out2d<uint32_t>(nq, k);
    py::array_t<float> d = out2d<float>(nq, k);
    const float *qp = q.data();
    uint32_t *ip = ids.mutable_data();
    float *dp = d.mutable_data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_flat_search_filtered(ix_, qp, nq, k, m.words, m.n_masks, m.of_query, ip, dp));
    }
    return py::make_tuple(ids, d);
  }
  void flat_search_filtered_device(uintptr_t q, uint64_t nq, uint32_t k, uintptr_t allow_words, uint32_t n_masks,
                                   uintptr_t mask_of_query, uintptr_t ids, uintptr_t dists, uintptr_t stream) {
    check(alaya_index_flat_search_filtered_device(ix_, dptr<const float>(q), nq, k, dptr<const uint32_t>(allow_words),
                                                  n_masks, dptr<const uint32_t>(mask_of_query), dptr<uint32_t>(ids),
                                                  dptr<float>(dists), dptr<void>(stream)));
  }
  // (allowed valid rows over the masks, row chunks of the last scan, its query tile, scan launches)
  py::tuple flat_filtered_last() const {
    uint64_t o[4] = {0, 0, 0, 0};
    check(alaya_index_flat_filtered_last(ix_, o));
    return py::make_tuple(o[0], o[1], o[2], o[3]);
  }
  // every valid (and allowed) row within `radius` (a number or one per query) of the query, by an exact scan
  // (alaya_index_flat_range_search): (counts[nq], ids[nq, max_results], dists[nq, max_results]); words / groups as
  // range_search's masks, None for no mask
  py::tuple flat_range_search(F32Array q, py::object radius, uint32_t max_results, py::object allow_words,
                              py::object mask_of_query) {
    const uint64_t nq = q.shape(0);
    U32Array words;
    const Masks m = parse_range_masks(allow_words, words, mask_of_query, rows(), nq);
    const std::vector<float> radii = parse_radii(radius, nq);
    if (max_results == 0 || max_results > 4096) throw py::value_error("max_results must be in 1..4096");
    py::array_t<uint32_t> ids = out2d<uint32_t>(nq, max_results);
    py::array_t<float> d = out2d<float>(nq, max_results);
    py::array_t<uint32_t> counts(static_cast<py::ssize_t>(nq));
    const float *qp = q.data();
    uint32_t *ip = ids.mutable_data();
    float *dp = d.mutable_data();
    uint32_t *np = counts.mutable_data();
    {
      py::gil_scoped_release nogil;
      check(alaya_index_flat_range_search(ix_, qp, nq, radii.data(), max_results, m.words, m.n_masks, m.of_query, np, ip, dp));
    }
    return py::make_tuple(counts, ids, d);
  }
  void flat_range_search_device(uintptr_t q, uint64_t nq, uintptr_t radii, uint32_t max_results, uintptr_t allow_words,
                                uint32_t n_masks, uintptr_t mask_of_query, uintptr_t counts, uintptr_t ids, uintptr_t dists,
                                uintptr_t stream) {
    check(alaya_index_flat_range_search_device(ix_, dptr<const float>(q), nq, dptr<const float>(radii), max_results,
                                               dptr<const uint32_t>(allow_words), n_masks,
                                               dptr<const uint32_t>(mask_of_query), dptr<uint32_t>(counts),
                                               dptr<uint32_t>(ids), dptr<float>(dists), dptr<void>(stream)));
  }
  // of the last mask: (eligible rows, row chunks, query tile, scan launches); over all masks: (eligible rows,
  // scan launches)
  py::tuple flat_range_last() const {
    uint64_t o[6] = {0, 0, 0, 0, 0, 0};
    check(alaya_index_flat_range_last(ix_, o));
    return py::make_tuple(o[0], o[1], o[2], o[3], o[4], o[5]);
  }
  int flat_contraction() const {
    int c = -1;
    check(alaya_index_flat_last_contraction(ix_, &c));
    return c;
  }
  void flat_diag(uintptr_t q, uint64_t nq, uint32_t k, int ablate, uintptr_t ids, uintptr_t dists,
                 uintptr_t flags, uintptr_t mc, uintptr_t stream) {
    check(alaya_index_flat_diag(ix_, dptr<const float>(q), nq, k, ablate, dptr<uint32_t>(ids), dptr<float>(dists),
                                dptr<uint32_t>(flags), dptr<uint32_t>(mc), dptr<void>(stream)));
  }
  py::tuple profile_search(F32Array q, uint32_t k, uint32_t ef, int space) {
    const uint64_t nq = q.shape(0);
    py::array_t<uint32_t> ids = out2d<uint32_t>(nq, k);
    py::array_t<uint32_t> c = out2d<uint32_t>(nq, 4);
    py::array_t<uint64_t> st = out2d<uint64_t>(nq, 8);
    check(alaya_index_profile_search(ix_, q.data(), nq, k, ef, space, ids.mutable_data(), c.mutable_data(),
                                     st.mutable_data()));
    return py::make_tuple(ids, c, st);
  }
  uint64_t device_bytes() const {
    uint64_t b = 0;
    check(alaya_index_info(ix_, nullptr, nullptr, nullptr, nullptr, &b));
    return b;
  }

 private:
  // the (nq, k) ids and distances and the (nq, 4) counters of a search, with their data pointers (taken
  // while the GIL is held)
  struct Results {
    py::array_t<uint32_t> ids;
    py::array_t<float> d;
    py::array_t<uint32_t> c;
    uint32_t *ip;
    float *dp;
    uint32_t *cp;
    Results(uint64_t nq, uint32_t k)
        : ids(out2d<uint32_t>(nq, k)), d(out2d<float>(nq, k)), c(out2d<uint32_t>(nq, 4)), ip(ids.mutable_data()),
          dp(d.mutable_data()), cp(c.mutable_data()) {}
  };
  uint64_t rows() const {  // the rows the masks of a filtered call cover
    uint64_t n = 0;
    check(alaya_index_info(ix_, &n, nullptr, nullptr, nullptr, nullptr));
    return n;
  }
};

}  // namespace alaya_py

PYBIND11_MODULE(_alayalitepy, m) {
  using namespace alaya_py;
  m.doc() = "AlayaLite MI355X engine";
  m.attr("__version__") = "0.1.0-mi355x";

  py::enum_<IndexType>(m, "IndexType")
      .value("FLAT", IndexType::FLAT)
      .value("HNSW", IndexType::HNSW)
      .value("NSG", IndexType::NSG)
      .value("FUSION", IndexType::FUSION)
      .export_values();
  py::enum_<MetricType>(m, "MetricType")
      .value("L2", MetricType::L2)
      .value("IP", MetricType::IP)
      .value("COS", MetricType::COS)
      .export_values();
  py::enum_<QuantizationType>(m, "QuantizationType")
      .value("NONE", QuantizationType::NONE)
      .value("SQ8", QuantizationType::SQ8)
      .value("SQ4", QuantizationType::SQ4)
      .value("RABITQ", QuantizationType::RABITQ)
      .export_values();

  py::class_<IndexParams>(m, "IndexParams")
      .def(py::init<>())
      .def(py::init([](IndexType it, py::dtype dt, py::dtype idt, QuantizationType qt, MetricType mt,
                       uint32_t cap) {
             IndexParams p;
             p.index_type_ = it;
             p.data_type_ = std::move(dt);
             p.id_type_ = std::move(idt);
             p.quantization_type_ = qt;
             p.metric_ = mt;
             p.capacity_ = cap;
             return p;
           }),
           py::arg("index_type_") = IndexType::HNSW, py::arg("data_type_") = py::dtype::of<float>(),
           py::arg("id_type_") = py::dtype::of<uint32_t>(),
           py::arg("quantization_type_") = QuantizationType::NONE,
           py::arg("metric_") = MetricType::L2, py::arg("capacity_") = 100000u)
      .def_readwrite("index_type_", &IndexParams::index_type_)
      .def_readwrite("data_type_", &IndexParams::data_type_)
      .def_readwrite("id_type_", &IndexParams::id_type_)
      .def_readwrite("quantization_type_", &IndexParams::quantization_type_)
      .def_readwrite("metric_", &IndexParams::metric_)
      .def_readwrite("capacity_", &IndexParams::capacity_);

  py::class_<PyIndexInterface, std::shared_ptr<PyIndexInterface>>(m, "PyIndexInterface")
      .def(py::init<IndexParams>(), py::arg("params"))
      .def("to_string", &PyIndexInterface::to_string)
      .def("fit", &PyIndexInterface::fit, py::arg("vectors"), py::arg("ef_construction"), py::arg("num_threads"),
           py::arg("builder") = "host")
      .def("search", &PyIndexInterface::search, py::arg("query"), py::arg("topk"), py::arg("ef"))
      .def("get_data_by_id", &PyIndexInterface::get_data_by_id, py::arg("id"))
      .def("insert", &PyIndexInterface::insert, py::arg("insert_data"), py::arg("ef"))
      .def("remove", &PyIndexInterface::remove, py::arg("id"))
      .def("add", &PyIndexInterface::add, py::arg("vectors"), py::arg("ef_construction"))
      .def("sq8_codes", &PyIndexInterface::sq8_codes)
      .def("sq8_range", &PyIndexInterface::sq8_range)
      .def("last_build_device_ms", &PyIndexInterface::last_build_device_ms)
      .def("batch_search", &PyIndexInterface::batch_search, py::arg("queries"), py::arg("topk"),
           py::arg("ef"), py::arg("num_threads"))
      .def("batch_search_with_distance", &PyIndexInterface::batch_search_with_distance,
           py::arg("queries"), py::arg("topk"), py::arg("ef"), py::arg("num_threads"))
      .def("exact_search", &PyIndexInterface::exact_search, py::arg("queries"), py::arg("topk"))
      .def("exact_search_filtered", &PyIndexInterface::exact_search_filtered, py::arg("queries"), py::arg("topk"),
           py::arg("allow_words"), py::arg("mask_of_query") = py::none())
      .def("exact_range_search", &PyIndexInterface::exact_range_search, py::arg("queries"), py::arg("radius"),
           py::arg("max_results"), py::arg("allow_words") = py::none(), py::arg("mask_of_query") = py::none())
      .def("save", &PyIndexInterface::save, py::arg("index_path"), py::arg("data_path"),
           py::arg("quant_path") = std::string())
      .def("load", &PyIndexInterface::load, py::arg("index_path"), py::arg("data_path"),
           py::arg("quant_path") = std::string())
      .def("filtered_search", &PyIndexInterface::filtered_search, py::arg("queries"), py::arg("topk"), py::arg("ef"),
           py::arg("allow_words"), py::arg("mask_of_query") = py::none(), py::arg("pool") = 0,
           py::arg("through") = false)
      .def("range_search", &PyIndexInterface::range_search, py::arg("queries"), py::arg("ef"), py::arg("radius"),
           py::arg("max_results"), py::arg("allow_words") = py::none(), py::arg("mask_of_query") = py::none(),
           py::arg("radius_mode") = false, py::arg("max_frontier") = 4096u, py::arg("more_append") = false)
      .def("range_search_sq8", &PyIndexInterface::range_search_sq8, py::arg("queries"), py::arg("ef"), py::arg("radius"),
           py::arg("code_radius"), py::arg("max_results"), py::arg("allow_words") = py::none(),
           py::arg("mask_of_query") = py::none(), py::arg("cand_append") = false)
      .def("last_range_candidates", &PyIndexInterface::last_range_candidates)
      .def("last_range_more", &PyIndexInterface::last_range_more)
      .def("last_through", &PyIndexInterface::last_through)
      .def("get_data_dim", &PyIndexInterface::get_data_dim)
      .def("get_data_num", &PyIndexInterface::get_data_num)
      .def("last_counters", &PyIndexInterface::last_counters)
      .def("set_hash_log2", &PyIndexInterface::set_hash_log2)
      .def("set_visited_mode", &PyIndexInterface::set_visited_mode)
      .def("set_helpers", &PyIndexInterface::set_helpers)
      .def("last_launch", &PyIndexInterface::last_launch)
      .def("help_stats", &PyIndexInterface::help_stats)
      .def("screen_stats", &PyIndexInterface::screen_stats)
      .def("scout_stats", &PyIndexInterface::scout_stats)
      .def("scout_policy_stats", &PyIndexInterface::scout_policy_stats)
      .def("last_plan", &PyIndexInterface::last_plan)
      .def("set_rerank_mode", &PyIndexInterface::set_rerank_mode)
      .def("rerank_mode", &PyIndexInterface::rerank_mode)
      .def("device_distances", &PyIndexInterface::device_distances)
      .def("graph_arrays", &PyIndexInterface::graph_arrays);


  py::class_<Graph, std::shared_ptr<Graph>>(m, "Graph")
      .def_static("build", &Graph::build, py::arg("data"), py::arg("metric") = 0, py::arg("R") = 32u,
                  py::arg("ef_construction") = 100u, py::arg("num_threads") = 1u, py::arg("seed") = 100u)
      .def_static("load", &Graph::load, py::arg("path"), py::arg("id_bytes") = 4)
      .def_static("from_arrays", &Graph::from_arrays, py::arg("l0"), py::arg("levels"), py::arg("upper_off"),
                  py::arg("upper_edges"), py::arg("upper_R"), py::arg("ep"), py::arg("eps") = py::none())
      .def("save", &Graph::save, py::arg("path"), py::arg("id_bytes") = 4, py::arg("capacity") = 0u)
      .def("arrays", &Graph::arrays);
  py::class_<DeviceIndex, std::shared_ptr<DeviceIndex>>(m, "DeviceIndex")
      .def(py::init<int>(), py::arg("device") = 0)
      .def("set_base", &DeviceIndex::set_base, py::arg("rows"), py::arg("metric") = 0, py::arg("valid") = py::none())
      .def("set_graph", &DeviceIndex::set_graph)
      .def("build_graph", &DeviceIndex::build_graph, py::arg("R") = 32, py::arg("ef_construction") = 100,
           py::arg("seed") = 100, py::arg("batch_div") = 0, py::arg("max_batch") = 0, py::arg("refine") = 2)
      .def("extend_graph", &DeviceIndex::extend_graph, py::arg("rows"), py::arg("ef_construction") = 100,
           py::arg("seed") = 100, py::arg("batch_div") = 0, py::arg("max_batch") = 0, py::arg("refine") = 2)
      .def("read_sq8", &DeviceIndex::read_sq8, py::arg("first"), py::arg("count"))
      .def("search", &DeviceIndex::search, py::arg("queries"), py::arg("k"), py::arg("ef"))
      .def("search_device", &DeviceIndex::search_device)
      .def("filtered_search", &DeviceIndex::filtered_search, py::arg("queries"), py::arg("k"), py::arg("ef"),
           py::arg("allow_words"), py::arg("mask_of_query") = py::none())
      .def("filtered_search_device", &DeviceIndex::filtered_search_device)
      .def("filtered_search_hop", &DeviceIndex::filtered_search_hop, py::arg("queries"), py::arg("k"), py::arg("ef"),
           py::arg("allow_words"), py::arg("mask_of_query") = py::none())
      .def("filtered_search_hop_device", &DeviceIndex::filtered_search_hop_device)
      .def("filtered_search_sq8", &DeviceIndex::filtered_search_sq8, py::arg("queries"), py::arg("k"), py::arg("ef"),
           py::arg("allow_words"), py::arg("mask_of_query") = py::none(), py::arg("pool") = 0,
           py::arg("rerank_queries") = py::none())
      .def("filtered_search_sq8_device", &DeviceIndex::filtered_search_sq8_device)
      .def("range_search", &DeviceIndex::range_search, py::arg("queries"), py::arg("ef"), py::arg("radius"),
           py::arg("max_results"), py::arg("allow_words") = py::none(), py::arg("mask_of_query") = py::none())
      .def("range_search_device", &DeviceIndex::range_search_device)
      .def("range_search_sq8", &DeviceIndex::range_search_sq8, py::arg("queries"), py::arg("ef"), py::arg("radius"),
           py::arg("code_radius"), py::arg("max_results"), py::arg("allow_words") = py::none(),
           py::arg("groups") = py::none(), py::arg("rerank_queries") = py::none())
      .def("range_search_sq8_device", &DeviceIndex::range_search_sq8_device)
      .def("range_search_radius", &DeviceIndex::range_search_radius, py::arg("queries"), py::arg("ef"), py::arg("radius"),
           py::arg("max_results"), py::arg("max_frontier") = 4096u, py::arg("allow_words") = py::none(),
           py::arg("mask_of_query") = py::none())
      .def("range_search_radius_device", &DeviceIndex::range_search_radius_device)
      .def("shard_search_device", &DeviceIndex::shard_search_device)
      .def("distances", &DeviceIndex::distances)
      .def("set_hash_log2", &DeviceIndex::set_hash_log2)
      .def("set_visited_mode", &DeviceIndex::set_visited_mode)
      .def("set_helpers", &DeviceIndex::set_helpers)
      .def("last_launch", &DeviceIndex::last_launch)
      .def("help_stats", &DeviceIndex::help_stats)
      .def("screen_stats", &DeviceIndex::screen_stats)
      .def("scout_stats", &DeviceIndex::scout_stats)
      .def("scout_policy_stats", &DeviceIndex::scout_policy_stats)
      .def("last_plan", &DeviceIndex::last_plan)
      .def("flat_search", &DeviceIndex::flat_search, py::arg("queries"), py::arg("k"))
      .def("flat_search_device", &DeviceIndex::flat_search_device)
      .def("flat_search_filtered", &DeviceIndex::flat_search_filtered, py::arg("queries"), py::arg("k"),
           py::arg("allow_words"), py::arg("mask_of_query") = py::none())
      .def("flat_search_filtered_device", &DeviceIndex::flat_search_filtered_device)
      .def("flat_filtered_last", &DeviceIndex::flat_filtered_last)
      .def("flat_range_search", &DeviceIndex::flat_range_search, py::arg("queries"), py::arg("radii"),
           py::arg("max_results"), py::arg("words") = py::none(), py::arg("groups") = py::none())
      .def("flat_range_search_device", &DeviceIndex::flat_range_search_device)
      .def("flat_range_last", &DeviceIndex::flat_range_last)
      .def("flat_diag", &DeviceIndex::flat_diag)
      .def("flat_contraction", &DeviceIndex::flat_contraction)
      .def("search_sq8_device", &DeviceIndex::search_sq8_device)
      .def("shard_search_sq8_device", &DeviceIndex::shard_search_sq8_device)
      .def("set_sq8", &DeviceIndex::set_sq8, py::arg("codes"), py::arg("min"), py::arg("max"), py::arg("order") = 2)
      .def("search_sq8", &DeviceIndex::search_sq8, py::arg("queries"), py::arg("k"), py::arg("ef"),
           py::arg("rerank") = 1, py::arg("rerank_queries") = py::none())
      .def("profile_search", &DeviceIndex::profile_search, py::arg("q"), py::arg("k"), py::arg("ef"),
           py::arg("space") = 0)
      .def("device_bytes", &DeviceIndex::device_bytes);
  m.def("sq8_train", [](F32Array data) {
    const uint32_t d = static_cast<uint32_t>(data.shape(1));
    py::array_t<float> mn(d), mx(d);
    check(alaya_sq8_train(data.data(), data.shape(0), d, mn.mutable_data(), mx.mutable_data()));
    return py::make_tuple(mn, mx);
  });
  m.def("sq8_encode", [](F32Array data, F32Array mn, F32Array mx, uint32_t threads) {
    py::array_t<uint8_t> codes({data.shape(0), data.shape(1)});
    check(alaya_sq8_encode(data.data(), data.shape(0), static_cast<uint32_t>(data.shape(1)), mn.data(), mx.data(),
                           codes.mutable_data(), threads));
    return codes;
  }, py::arg("data"), py::arg("min"), py::arg("max"), py::arg("num_threads") = 1u);
  m.def("host_sq8_order", &host_sq8_order);
  // the batch ends of the build schedule of rows [start, n) (alaya_build_batches; no device needed)
  m.def("build_batches", [](U32Array levels, uint64_t start, uint32_t ep, uint32_t batch_div, uint32_t max_batch) {
    if (levels.ndim() != 1) throw py::value_error("levels must be 1D");
    const uint64_t n = levels.shape(0);
    uint64_t nb = 0;
    check(alaya_build_batches(levels.data(), n, start, ep, batch_div, max_batch, nullptr, &nb));
    py::array_t<uint64_t> ends(static_cast<py::ssize_t>(nb));
    check(alaya_build_batches(levels.data(), n, start, ep, batch_div, max_batch, ends.mutable_data(), &nb));
    return ends;
  }, py::arg("levels"), py::arg("start") = 1, py::arg("ep") = 0, py::arg("batch_div") = 0, py::arg("max_batch") = 0);
  m.def("build_info", [] { return std::string(alaya_build_info()); });
  m.def("screen_lower_bound", [](F32Array d_tilde, F32Array e_row, uint32_t dim) {
    if (d_tilde.size() != e_row.size()) throw std::invalid_argument("d_tilde and e_row differ in size");
    py::array_t<float> out(d_tilde.size());
    check(alaya_screen_lower_bound(d_tilde.data(), e_row.data(), static_cast<uint64_t>(d_tilde.size()), dim,
                                   out.mutable_data()));
    return out;
  });
  // the 8-bit screening copy on the host: (codes, header (e_row, lo, scale, 0), values the codes stand for)
  m.def("screen_u8_quantize", [](F32Array rows) {
    if (rows.ndim() != 2) throw std::invalid_argument("rows must be 2-D");
    py::array_t<uint8_t> codes({rows.shape(0), rows.shape(1)});
    py::array_t<float> header({rows.shape(0), static_cast<py::ssize_t>(4)});
    py::array_t<float> values({rows.shape(0), rows.shape(1)});
    check(alaya_screen_u8_quantize(rows.data(), static_cast<uint64_t>(rows.shape(0)), static_cast<uint32_t>(rows.shape(1)),
                                   codes.mutable_data(), header.mutable_data(), values.mutable_data()));
    return py::make_tuple(codes, header, values);
  });
  // the integer screen's bound on the host, pair i = (queries[i], rows[i]): (d_in <= ||q^ - y^||^2,
  // e_sum >= ||x - y^|| + ||q - q^||, the bound, sums (n x 5: A1, A2, C1, C2, AC))
  m.def("screen_int_bound", [](F32Array queries, F32Array rows) {
    if (rows.ndim() != 2 || queries.ndim() != 2 || rows.shape(0) != queries.shape(0) || rows.shape(1) != queries.shape(1))
      throw std::invalid_argument("queries and rows must be 2-D of one shape");
    py::array_t<float> d_in(rows.shape(0)), e_sum(rows.shape(0)), bound(rows.shape(0));
    py::array_t<uint32_t> sums({rows.shape(0), static_cast<py::ssize_t>(5)});
    check(alaya_screen_int_bound(queries.data(), rows.data(), static_cast<uint64_t>(rows.shape(0)),
                                 static_cast<uint32_t>(rows.shape(1)), d_in.mutable_data(), e_sum.mutable_data(),
                                 bound.mutable_data(), sums.mutable_data()));
    return py::make_tuple(d_in, e_sum, bound, sums);
  });
  // the exact filtered scan's launch plan on the host (alaya_flat_filtered_plan): (rows per chunk, chunks,
  // query tile, queries per scan launch, partial-list bytes)
  m.def("flat_filtered_plan", [](uint64_t n_allowed, uint64_t nq, uint32_t k, uint32_t stride, uint32_t cus) {
    uint64_t o[5] = {0, 0, 0, 0, 0};
    check(alaya_flat_filtered_plan(n_allowed, nq, k, stride, cus, o));
    return py::make_tuple(o[0], o[1], o[2], o[3], o[4]);
  }, py::arg("n_allowed"), py::arg("nq"), py::arg("k"), py::arg("stride"), py::arg("cus"));
  // the exact range scan's launch plan on the host (alaya_flat_range_plan): (rows per chunk, chunks, query
  // tile, queries per scan launch, stored hits per (chunk, query), staging bytes)
  m.def("flat_range_plan", [](uint64_t n_eligible, uint64_t nq, uint32_t max_results, uint32_t stride, uint32_t cus) {
    uint64_t o[6] = {0, 0, 0, 0, 0, 0};
    check(alaya_flat_range_plan(n_eligible, nq, max_results, stride, cus, o));
    return py::make_tuple(o[0], o[1], o[2], o[3], o[4], o[5]);
  }, py::arg("n_eligible"), py::arg("nq"), py::arg("max_results"), py::arg("stride"), py::arg("cus"));
  // the flat search's inner-product bound on the host (flat_bound.h): slack per query, and the test
  m.def("flat_ip_slack", [](int contraction, uint32_t k_acc, F32Array q_norm2, CArray<int> q_exp, float b_max,
                            int base_exp) {
    if (q_exp.size() != 0 && q_exp.size() != q_norm2.size()) throw std::invalid_argument("q_norm2 and q_exp differ in size");
    py::array_t<float> out(q_norm2.size());
    check(alaya_flat_ip_slack(contraction, k_acc, q_norm2.data(), q_exp.size() ? q_exp.data() : nullptr,
                              static_cast<uint64_t>(q_norm2.size()), b_max, base_exp, out.mutable_data()));
    return out;
  }, py::arg("contraction"), py::arg("k_acc"), py::arg("q_norm2"), py::arg("q_exp"), py::arg("b_max"),
     py::arg("base_exp") = 0);
  m.def("flat_ip_proven", [](F32Array kth_d, F32Array cutoff, F32Array slack) {
    if (kth_d.size() != cutoff.size() || kth_d.size() != slack.size()) throw std::invalid_argument("sizes differ");
    py::array_t<uint8_t> out(kth_d.size());
    check(alaya_flat_ip_proven(kth_d.data(), cutoff.data(), slack.data(), static_cast<uint64_t>(kth_d.size()),
                               out.mutable_data()));
    return out;
  }, py::arg("kth_d"), py::arg("cutoff"), py::arg("slack"));
  // a float32 copy with each row normalised as fit does for COS (alaya_amd::normalize_row)
  m.def("normalize_rows", [](F32Array a) {
    if (a.ndim() != 2) throw std::invalid_argument("normalize_rows needs a 2D array");
    py::array_t<float> out({a.shape(0), a.shape(1)});
    if (a.size()) std::memcpy(out.mutable_data(), a.data(), static_cast<size_t>(a.size()) * 4);
    for (py::ssize_t i = 0; i < a.shape(0); ++i)
      alaya_amd::normalize_row(out.mutable_data() + i * a.shape(1), static_cast<size_t>(a.shape(1)));
    return out;
  }, py::arg("array"));
  // the search kernel chosen for a request: ((space, chunks, mode), features this shape has kernels for)
  m.def("search_variant", [](uint32_t dim, bool ip, int sq8_order, bool generic, uint32_t wanted_mode) {
    int space = 0;
    uint32_t chunks = 0, mode = 0, has = 0;
    check(alaya_search_variant(dim, ip, sq8_order, generic, wanted_mode, &space, &chunks, &mode, &has));
    return py::make_tuple(py::make_tuple(space, chunks, mode), has);
  }, py::arg("dim"), py::arg("ip"), py::arg("sq8_order"), py::arg("generic"), py::arg("wanted_mode"));
  // the list of search kernel variants: (space, chunks, mode, l2_only) per row
  m.def("search_variants", [] {
    py::list rows;
    uint32_t count = 1;
    for (uint32_t i = 0; i < count; ++i) {
      int space = 0, l2_only = 0;
      uint32_t chunks = 0, mode = 0;
      check(alaya_search_variant_at(i, &space, &chunks, &mode, &l2_only, &count));
      rows.append(py::make_tuple(space, chunks, mode, l2_only != 0));
    }
    return rows;
  });
  m.def("device_count", [] {
    int c = 0;
    check(alaya_device_count(&c));
    return c;
  });
  m.def("hbm_stream_read", [](int device, uint64_t bytes, int iters) {
    double gbs = 0.0;
    check(alaya_hbm_stream_read(device, bytes, iters, &gbs));
    return gbs;
  }, py::arg("device") = 0, py::arg("bytes") = 4ull << 30, py::arg("iters") = 5);
  // a CU-masked stream (handle as an int, for torch.cuda.ExternalStream) and its release
  m.def("stream_create_reserving", [](int device, uint32_t reserved_cus) {
    void *s = nullptr;
    check(alaya_stream_create_reserving(device, reserved_cus, &s));
    return reinterpret_cast<uintptr_t>(s);
  }, py::arg("device"), py::arg("reserved_cus"));
  m.def("stream_destroy", [](uintptr_t s) { check(alaya_stream_destroy(dptr<void>(s))); });
}
