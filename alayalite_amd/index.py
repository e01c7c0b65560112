"""Index: one vector index whose search runs on the MI355X (mirrors alayalite/index.py,
python/src/alayalite/index.py:35-231; same signatures, same ValueError/RuntimeError behaviour)."""

from __future__ import annotations

import os

import numpy as np

from ._native import PyIndexInterface as _PyIndexInterface
from .common import VectorLike, VectorLikeBatch, _assert
from .schema import IndexParams, load_schema
from .utils import exact_range_args, pack_allow, range_csr


class Index:
    """A vector index: ``fit`` builds the HNSW graph (host) and uploads rows + graph to HBM; all
    ``search`` / ``batch_search`` calls run the device graph search kernel."""

    def __init__(self, name: str = "default", params: IndexParams = None):
        self.__name = name
        self.__params = params if params is not None else IndexParams()
        self.__index = None
        self.__is_initialized = False
        self.__dim = None

    def get_params(self) -> IndexParams:
        return self.__params

    def get_data_by_id(self, vector_id: int) -> VectorLike:
        return self.__index.get_data_by_id(vector_id)

    def fit(self, vectors: VectorLikeBatch, ef_construction: int = 100, num_threads: int = 1,
            builder: str = "host"):
        """index.py:75-99.  builder="host" builds the graph with the reference's HNSWBuilder restated
        on the host (num_threads=1 gives the reference's graph exactly); builder="gpu" builds it on the
        MI355X by batched insertion (alaya_index_build_graph) -- same algorithm, orders of magnitude
        faster at 1M+ rows, graph not identical to the sequential one."""
        _assert(builder in ("host", "gpu"), "builder must be 'host' or 'gpu'")
        if self.__is_initialized:
            raise RuntimeError("An index can be only fitted once")
        _assert(vectors.ndim == 2, "vectors must be a 2D array")
        data_type = np.array(vectors).dtype
        if self.__params.data_type is None:
            self.__params.data_type = data_type
        elif self.__params.data_type != data_type:
            raise ValueError(f"Data type mismatch: {self.__params.data_type} vs {data_type}")
        self.__params.fill_none_values()
        self.__dim = vectors.shape[1]
        self.__index = _PyIndexInterface(self.__params.to_cpp_params())
        self.__is_initialized = True
        self.__index.fit(vectors, ef_construction, num_threads, builder)

    def insert(self, vectors: VectorLike, ef: int = 100):
        _assert(self.__index is not None, "Index is not init yet")
        _assert(vectors.ndim == 1, "vectors must be a 1D array")
        _assert(vectors.shape[0] == self.__dim,
                "vectors dimension must match the dimension of the vectors used to fit the index."
                f"fit data dimension: {self.__dim}, vectors dimension: {vectors.shape[0]}")
        ret = self.__index.insert(vectors, ef)
        full = ret == -1 or (self.__params.id_type == np.uint32 and ret == 0xFFFFFFFF) or (
            self.__params.id_type == np.uint64 and ret == 0xFFFFFFFFFFFFFFFF)
        if full:
            raise RuntimeError("The index is full, cannot insert more vectors")
        return ret

    def add(self, vectors: VectorLikeBatch, ef_construction: int = 100) -> VectorLike:
        """Append the rows of ``vectors`` (2-D, the index's width and dtype) in bulk and return their
        ids, ``n0 .. n0 + m - 1`` in the index's id type.  The graph grows on the MI355X by continuing
        the batched build of ``fit(builder="gpu")`` (same seed, schedule and refine passes) from the
        graph the index holds, whatever built it and whatever ``insert`` / ``remove`` did to it; when
        ``n0`` is a batch boundary of that build, ``fit(first n0) + add(rest)`` is ``fit(all)`` exactly.
        No new row links to a removed row.  COS rows are normalised in place, as ``fit`` does.  An SQ8
        index encodes the new rows with the quantizer fitted at ``fit``: it is not retrained, so values
        outside a dimension's fitted range clamp.  ``m == 0`` is a no-op; past the index capacity the
        call raises RuntimeError and adds nothing.  One call per block of rows: every call regrows the
        device buffers and downloads the whole graph."""
        _assert(self.__index is not None, "Index is not init yet")
        vectors = np.asarray(vectors)
        _assert(vectors.ndim == 2, "vectors must be a 2D array")
        _assert(vectors.shape[1] == self.__dim,
                "vectors dimension must match the dimension of the vectors used to fit the index."
                f"fit data dimension: {self.__dim}, vectors dimension: {vectors.shape[1]}")
        if self.__params.data_type != vectors.dtype:
            raise ValueError(f"Data type mismatch: {self.__params.data_type} vs {vectors.dtype}")
        n0, m = self.__index.get_data_num(), vectors.shape[0]
        if n0 + m > self.__params.capacity:
            raise RuntimeError("The index is full, cannot insert more vectors")
        if m:
            self.__index.add(vectors, ef_construction)
        return np.arange(n0, n0 + m, dtype=self.__params.id_type)

    def remove(self, vector_id: int) -> None:
        _assert(self.__index is not None, "Index is not init yet")
        self.__index.remove(vector_id)

    def _check_queries(self, queries, ndim: int, what: str):
        _assert(self.__index is not None, "Index is not init yet")
        _assert(queries.ndim == ndim, f"{what} must be a {ndim}D array")
        got = queries.shape[-1]
        _assert(got == self.__dim,
                "query dimension must match the dimension of the vectors used to fit the index."
                f"fit data dimension: {self.__dim}, query dimension: {got}")

    def _masks(self, allow, groups, nq: int):
        """``allow`` and ``groups`` of the masked searches, checked, as (mask words, uint32 groups or None)."""
        allow = np.asarray(allow)
        _assert(allow.ndim in (1, 2), "allow must have shape (n,) or (G, n)")
        words = pack_allow(allow, self.get_data_num())
        if groups is None:
            _assert(words.shape[0] == 1, "groups is required with more than one mask")
        else:
            groups = np.asarray(groups)
            _assert(groups.shape == (nq,), "groups must have shape (nq,)")
            _assert(np.issubdtype(groups.dtype, np.integer), "groups must be integers")
            _assert(groups.size == 0 or (groups.min() >= 0 and groups.max() < words.shape[0]),
                    "groups must be below the number of masks")
            groups = np.ascontiguousarray(groups, np.uint32)
        return words, groups

    def search(self, query: VectorLike, topk: int, ef_search: int = 100) -> VectorLike:
        self._check_queries(query, 1, "query")
        return self.__index.search(query, topk, ef_search)

    def batch_search(self, queries: VectorLikeBatch, topk: int, ef_search: int = 100,
                     num_threads: int = 1) -> VectorLikeBatch:
        self._check_queries(queries, 2, "queries")
        return self.__index.batch_search(queries, topk, ef_search, num_threads)

    def batch_search_with_distance(self, queries: VectorLikeBatch, topk: int, ef_search: int = 100,
                                   num_threads: int = 1):
        self._check_queries(queries, 2, "queries")
        return self.__index.batch_search_with_distance(queries, topk, ef_search, num_threads)

    def get_dim(self):
        return self.__dim

    def get_dtype(self):
        return self.__params.data_type

    # ---- engine extras (not in the reference API) -------------------------------------------
    def native(self):
        """The underlying PyIndexInterface (device counters, graph arrays, tuning)."""
        return self.__index

    def exact_search(self, queries: VectorLikeBatch, topk: int, allow=None, groups=None):
        """The exact top-k of each query over the rows the index holds (valid rows only, the index's
        metric in f32, ties by id): the flat MFMA search on the device rows -- the ground truth for
        the recall of ``batch_search`` at some ``ef_search``.  Returns (ids, distances); slots past the
        valid rows hold (the id type's maximum, FLT_MAX).  1 <= topk <= 224, float32 data.

        With ``allow`` (``filtered_search``'s masks: a bool array of shape (n,), n = ``get_data_num()``,
        or (G, n) with ``groups`` of shape (nq,), the mask of each query) the answer is the exact
        top-k among the valid rows the query's mask allows, same order, same distance bits, same
        empty slots; an SQ8 index is scanned on its float32 rows.  This skips the graph and scans
        the allowed rows, each one reused across a tile of queries, so its cost grows with
        allowed rows x queries: it is meant for small allowed shares, where the graph
        ``filtered_search`` loses recall.  Above the measured crossover (a few per cent of the rows,
        DESIGN.md section 3, Round 16) the graph ``filtered_search`` or the unmasked
        ``exact_search`` is faster."""
        self._check_queries(queries, 2, "queries")
        if allow is None:
            _assert(groups is None, "groups needs allow")
            return self.__index.exact_search(queries, topk)
        words, groups = self._masks(allow, groups, queries.shape[0])
        return self.__index.exact_search_filtered(queries, topk, words, groups)

    def get_data_num(self) -> int:
        """Rows the index holds, removed ones included: the length of a ``filtered_search`` mask."""
        _assert(self.__index is not None, "Index is not init yet")
        return self.__index.get_data_num()

    def filtered_search(self, queries: VectorLikeBatch, topk: int, ef_search: int = 100, allow=None, groups=None,
                        rerank_pool=None, expand="plain"):
        """The ``topk`` nearest rows among those a mask allows.  The graph traversal is ``batch_search``'s
        at ``ef_search``; every distance it computes for a valid, allowed row is offered to a result
        pool of ``topk`` entries, so the answer draws on all of them and not only on the ``ef_search``
        rows the traversal keeps.  ``allow``: bool array of shape (n,), n = ``get_data_num()``, or
        (G, n) with ``groups`` of shape (nq,), the mask (an int below G) of each query.  Returns
        (ids, distances); slots the allowed rows did not fill hold (the id type's maximum, FLT_MAX).
        1 <= topk <= 224.

        An SQ8 index traverses its codes, as its ``batch_search`` does, keeps the ``rerank_pool``
        allowed rows nearest by code distance (``topk <= rerank_pool <= 224``; None =
        ``min(224, max(topk, ef_search))``) and returns the ``topk`` of them nearest by exact float32
        distance, ties by id; the distances returned are the exact ones.  On an unquantized index
        ``rerank_pool`` must stay None.

        ``expand="through"`` (float32 indexes only) selects a second traversal.  A neighbour that is not
        allowed (or was removed) is neither measured nor kept: the search marks it visited and walks its
        own level-0 row instead, one level deep, for allowed rows not yet visited.  So the pool of
        ``ef_search`` entries holds allowed rows only, beside the entry point, and ``ef_search`` keeps its
        usual meaning; with every row allowed the answer is that of ``expand="plain"``.  It is meant for
        small and middling allowed shares, where the plain traversal loses recall (GIST-shaped 1M x 960,
        ef 387: recall@10 0.97 - 0.99 at shares 0.5 .. 0.05 against 0.93 .. 0.82), and it is not free: it
        reads one adjacency row per row stepped through (``native().last_through()``), which makes the
        launch 2x - 7x the plain one at the same ``ef_search``, and at a share of 0.5 it also computes
        about five times the plain traversal's distances, so the caller chooses (a smaller ``ef_search``
        often suffices).  Below a share of about 0.1 ``exact_search(allow=)`` is exact and faster
        ("Round 17")."""
        self._check_queries(queries, 2, "queries")
        _assert(allow is not None, "allow is required")
        _assert(expand in ("plain", "through"), "expand must be 'plain' or 'through'")
        through = expand == "through"
        if through:
            _assert((self.__params.quantization_type or "none").lower() != "sq8" and rerank_pool is None,
                    "expand='through' searches f32 indexes only (no SQ8 codes, no rerank_pool)")
        pool = 0
        if rerank_pool is not None:
            _assert((self.__params.quantization_type or "none").lower() == "sq8", "rerank_pool applies to SQ8 indexes only")
            pool = int(rerank_pool)
            _assert(topk <= pool <= 224, "rerank_pool must be in topk..224")
        words, groups = self._masks(allow, groups, queries.shape[0])
        return self.__index.filtered_search(queries, topk, ef_search, words, groups, pool, through)

    def range_search(self, queries: VectorLikeBatch, radius, ef_search: int = 100, max_results: int = 1024,
                     allow=None, groups=None, _chunk=None, expand="fixed", max_frontier: int = 4096, slack=None):
        """Every row within distance ``radius`` of each query, among the rows the graph traversal measures.
        The traversal is ``batch_search``'s at ``ef_search``; the radius does not steer it.  Every distance it
        computes for a valid row (and, with ``allow`` / ``groups`` as in ``filtered_search``, an allowed one)
        that is ``<= radius`` is a hit -- all of them, not only the ``ef_search`` rows the traversal keeps.
        The distance is the index's own: squared L2, ``-(q.b)`` for IP, the same on normalised rows and
        queries for COS, so ``radius=-0.8`` on a COS index means cosine >= 0.8.  ``radius`` is a number or
        an array of shape (nq,), not NaN.

        Returns ``(lims, ids, dists, counts)``: ``lims`` is int64 of length nq + 1 and query i's rows are
        ``ids[lims[i]:lims[i + 1]]`` (the index's id type) with ``dists`` beside them, ordered by
        (distance, id).  ``counts[i]`` (uint32) is the number of hits, not capped, and
        ``lims[i + 1] - lims[i] == min(counts[i], max_results)``.  ``counts[i] > max_results`` means the
        list is truncated: it then holds the first ``max_results`` hits the traversal met, NOT the nearest
        ones -- raise ``max_results`` (1..4096) or lower the radius.  A removed row is never returned.
        On a float32 index ``slack`` must stay None.

        An SQ8 index needs ``slack``: a number or an array of shape (nq,), >= 0, not NaN.  Its traversal
        measures code distances, as its ``batch_search`` does, and those differ from the exact ones in both
        directions.  So a valid, allowed row the traversal measures is a *candidate* when its code distance is
        ``<= float32(radius) + float32(slack)``; the first ``max_results`` candidates to turn up are measured
        exactly on their float32 rows, and those with exact distance ``<= radius`` are the hits, returned with
        their exact distances.  Here ``counts[i]`` is the number of hits returned, so
        ``lims[i + 1] - lims[i] == counts[i]``, and truncation shows elsewhere:
        ``native().last_range_candidates()[i] > max_results`` (uint32, shape (nq,), the candidates of the last
        call) means candidates past the first ``max_results`` were never measured exactly.  ``slack=0`` misses
        rows whose code distance overstates the exact one; a larger slack admits them at the price of more
        candidates to rerank; ``slack=np.inf`` makes every valid, allowed measured row a candidate.  No bound on
        the code error is assumed: the slack is the caller's choice ("Round 21").
        ``expand="radius"`` is refused on an SQ8 index.

        ``expand="radius"`` lets the radius steer the search.  The traversal above runs first, unchanged;
        ``ef_search`` now only says where the flood fill starts.  Then every valid row measured within the
        radius -- allowed or not -- is expanded in the order it turned up: its unvisited neighbours are
        measured, the ones within the radius are hits (if allowed) and are expanded in their turn, until no
        new row within the radius turns up.  The result is the in-radius region of the graph that the
        traversal reached, so a small ``ef_search`` suffices where ``expand="fixed"`` needs a guess that
        grows with the radius ("Round 20").  At most ``max_frontier`` (1..16384) rows
        per query are expanded this way, the first to turn up.  ``native().last_range_more()`` is a uint32
        array of shape (nq, 2) for the last call: column 0 the rows within the radius that turned up,
        column 1 the distances the continuation computed.  There are now two truncations:
        ``counts[i] > max_results`` as above, and ``last_range_more()[i, 0] > max_frontier`` -- rows past
        the first ``max_frontier`` were counted and returned but not expanded, so rows behind them may be
        missing.  A huge radius makes the continuation read up to ``max_frontier`` adjacency rows and
        measure up to ``max_frontier x R`` rows per query: it is the radius that bounds the work.
        ``expand="fixed"`` (the default) is the call without the keyword, bit for bit."""
        self._check_queries(queries, 2, "queries")
        _assert(expand in ("fixed", "radius"), "expand must be 'fixed' or 'radius'")
        radius_mode = expand == "radius"
        _assert(1 <= max_frontier <= 16384, "max_frontier must be in 1..16384")
        sq8 = (self.__params.quantization_type or "none").lower() == "sq8"
        _assert(not (sq8 and radius_mode), "expand='radius' searches f32 indexes only: this index has SQ8 codes")
        _assert(not sq8 or slack is not None,
                "range_search of an index with SQ8 codes measures code distances: pass slack= (0 or more)")
        _assert(sq8 or slack is None, "slack applies to SQ8 indexes only")
        _assert(1 <= max_results <= 4096, "max_results must be in 1..4096")
        _assert(ef_search >= 1, "ef_search must be >= 1")
        nq = queries.shape[0]
        if sq8:
            slacks = np.asarray(slack, np.float32)
            _assert(slacks.shape in ((), (nq,)), "slack must be a number or have shape (nq,)")
            _assert(not np.isnan(slacks).any() and (slacks >= 0).all(), "slack must be >= 0 and not NaN")
        radii = np.asarray(radius, np.float32)
        _assert(radii.shape in ((), (nq,)), "radius must be a number or have shape (nq,)")
        _assert(not np.isnan(radii).any(), "radius must not be NaN")
        radii = np.ascontiguousarray(np.broadcast_to(radii, (nq,)))
        if sq8:
            with np.errstate(invalid="ignore"):  # (-inf + inf: refused below)
                code_radii = np.ascontiguousarray(radii + np.broadcast_to(slacks, (nq,)), np.float32)
            _assert(not np.isnan(code_radii).any(), "radius + slack must not be NaN")
        words = None
        if allow is None:
            _assert(groups is None, "groups needs allow")
        else:
            words, groups = self._masks(allow, groups, nq)
        # chunks of queries: at most 2^26 padded result (and frontier) slots per call
        widest = max(max_results, max_frontier) if radius_mode else max_results
        step = max(1, (1 << 26) // widest) if _chunk is None else int(_chunk)
        parts = []
        for lo in range(0, nq, step):
            hi = min(nq, lo + step)
            if sq8:
                counts, ids, dists, _ = self.__index.range_search_sq8(queries[lo:hi], ef_search, radii[lo:hi],
                                                                      code_radii[lo:hi], max_results, words,
                                                                      None if groups is None else groups[lo:hi], lo > 0)
            elif radius_mode:
                counts, ids, dists, _ = self.__index.range_search(queries[lo:hi], ef_search, radii[lo:hi], max_results,
                                                                  words, None if groups is None else groups[lo:hi], True,
                                                                  max_frontier, lo > 0)
            else:
                counts, ids, dists, _ = self.__index.range_search(queries[lo:hi], ef_search, radii[lo:hi], max_results,
                                                                  words, None if groups is None else groups[lo:hi])
            parts.append((counts,) + range_csr(counts, ids, dists, max_results)[1:])
        if not parts:
            return (np.zeros(1, np.int64), np.zeros(0, self.__params.id_type), np.zeros(0, np.float32),
                    np.zeros(0, np.uint32))
        counts = np.concatenate([p[0] for p in parts])
        lims = np.zeros(nq + 1, np.int64)
        np.cumsum(np.minimum(counts.astype(np.int64), max_results), out=lims[1:])
        return lims, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), counts

    def exact_range_search(self, queries: VectorLikeBatch, radius, max_results: int = 1024, allow=None, groups=None,
                           _chunk=None):
        """Every row within distance ``radius`` of each query, exactly: a scan of the rows, no graph.  A row
        is a hit when it is valid (not removed), allowed by the query's mask (``allow`` / ``groups`` as in
        ``filtered_search``; no ``allow`` = every row) and its distance is ``<= radius``, inclusive.  The
        distance is ``exact_search``'s, bit for bit: the index's metric in f32 (squared L2, ``-(q.b)`` for
        IP, the same on normalised rows and queries for COS); an SQ8 index is scanned on its float32 rows.
        ``radius`` is a number or an array of shape (nq,), not NaN; ``-inf`` matches nothing, ``inf`` every
        eligible row.  This is the ground truth for the range recall of ``range_search``, and the call for
        near-duplicate, threshold-join and clustering queries that need all of the rows.

        Returns ``range_search``'s form ``(lims, ids, dists, counts)``: ``counts[i]`` (uint32) is the exact
        number of hits, never capped; query i's rows ``ids[lims[i]:lims[i + 1]]`` are
        ``min(counts[i], max_results)`` of them ordered by (distance, id).  ``counts[i] > max_results``
        (1..4096) means the list is truncated: it then holds the ``max_results`` hits with the SMALLEST IDS,
        not the nearest ones (the scan meets rows in ascending id) -- lower the radius, or split the rows
        with masks.  The result depends on the inputs alone.

        The cost is eligible rows x queries: it is the f32 scan of ``exact_search(allow=)``, each row reused
        across a tile of 16 queries, and not the MFMA flat scan of the unmasked ``exact_search``
        ("Round 22")."""
        self._check_queries(queries, 2, "queries")
        nq = queries.shape[0]
        radii = exact_range_args(nq, radius, max_results, allow, groups)
        words = None
        if allow is not None:
            words, groups = self._masks(allow, groups, nq)
        # chunks of queries: at most 2^26 padded result slots per call
        step = max(1, (1 << 26) // max_results) if _chunk is None else int(_chunk)
        parts = []
        for lo in range(0, nq, step):
            hi = min(nq, lo + step)
            counts, ids, dists = self.__index.exact_range_search(queries[lo:hi], radii[lo:hi], max_results, words,
                                                                 None if groups is None else groups[lo:hi])
            parts.append((counts,) + range_csr(counts, ids, dists, max_results)[1:])
        if not parts:
            return (np.zeros(1, np.int64), np.zeros(0, self.__params.id_type), np.zeros(0, np.float32),
                    np.zeros(0, np.uint32))
        counts = np.concatenate([p[0] for p in parts])
        lims = np.zeros(nq + 1, np.int64)
        np.cumsum(np.minimum(counts.astype(np.int64), max_results), out=lims[1:])
        return lims, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), counts

    def save(self, url) -> dict:
        os.makedirs(url, exist_ok=True)
        p = self.__params
        self.__index.save(p.index_path(url), p.data_path(url), p.quant_path(url))
        return {"type": "index", "index": p.to_json_dict()}

    @classmethod
    def load(cls, url, name):
        index_url = os.path.join(url, name)
        if not os.path.exists(index_url):
            raise RuntimeError("The index file does not exist")
        params = IndexParams.from_str_dict(load_schema(os.path.join(index_url, "schema.json"))["index"])
        instance = cls(name, params)
        instance.__index = _PyIndexInterface(params.to_cpp_params())
        instance.__index.load(params.index_path(index_url), params.data_path(index_url), params.quant_path(index_url))
        instance.__is_initialized = True
        instance.__dim = instance.__index.get_data_dim()
        return instance
