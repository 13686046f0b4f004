"""The edge list: the pairs of a collection within a threshold, without the dense matrix.

Owns ``SparseEdges``, its routes ``edges_de_novo`` and ``edges_extend`` with their guard (``_guard_edges``, which the tree's
route shares) and ``merge_edge_lists``.  Its adjacency file is written by ``matrix.edges_to_adjacency``."""

import numpy as np

from phamclust_amd.symmatrix import _square_matrix
from phamclust_amd.routes import _de_novo_route, _extend_fill, _extend_plan
from phamclust_amd.results._common import _grown_positions, _live_row_pairs, _passes, _positions_without, _smallest_member_labels


class SparseEdges:
    """The edges of a matrix that pass a threshold -- ``weight <= threshold`` on distances, ``>= threshold`` on similarities -- as
    three parallel arrays over ``nodes``: ``source[e] < target[e]`` (indices into ``nodes``), sorted by target, then source, and
    ``weight[e]``.  It is the sparse form the reference derives from its dense matrix twice: ``matrix_to_adjacency(...,
    skip_zero=True)`` (matrix.py:536-551) and ``SymMatrix.nearest_neighbors`` (matrix.py:265-296); ``edges_de_novo`` fills it on the
    GPU without the dense matrix.  The diagonal is implied: ``1.0 - is_distance`` (matrix.py:467-468)."""

    def __init__(self, nodes, source, target, weight, is_distance=True, threshold=None):
        self.nodes = list(nodes)
        self.source = np.ascontiguousarray(source, dtype=np.int32)
        self.target = np.ascontiguousarray(target, dtype=np.int32)
        self.weight = np.ascontiguousarray(weight, dtype=np.float64)
        if not (self.source.shape == self.target.shape == self.weight.shape and self.source.ndim == 1):
            raise ValueError("source, target and weight must be three 1-D arrays of one length")
        self.is_distance = bool(is_distance)
        self.threshold = threshold
        self._slot = None
        self._incident = None

    @classmethod
    def from_dense(cls, matrix, threshold):
        """The edges of a filled ``SymMatrix`` within ``threshold``, in its current node order (tests and small inputs)."""
        data = matrix._ordered()
        s, t = np.triu_indices(len(matrix), k=1)
        w = data[s, t]
        keep = np.flatnonzero(_passes(w, threshold, matrix.is_distance))
        keep = keep[np.lexsort((s[keep], t[keep]))]
        return cls(matrix.nodes, s[keep], t[keep], w[keep], is_distance=matrix.is_distance, threshold=threshold)

    def __len__(self):
        return int(self.weight.shape[0])

    def _adjacency_order(self):
        """(source, target, weight) index / value arrays in the reference's adjacency order (matrix.py:368-379, 536-551):
        source-major, each node's self-edge first, then its targets ascending -- one stable argsort of the source over the
        (target, source)-sorted edges behind the diagonal."""
        n = len(self.nodes)
        loop = np.arange(n, dtype=np.int32)
        src = np.concatenate([loop, self.source])
        order = np.argsort(src, kind="stable")
        tgt = np.concatenate([loop, self.target])[order]
        w = np.concatenate([np.full(n, 0.0 if self.is_distance else 1.0), self.weight])[order]
        return np.ascontiguousarray(src[order]), np.ascontiguousarray(tgt), np.ascontiguousarray(w)

    def __iter__(self):
        src, tgt, w = self._adjacency_order()
        for i, j, x in zip(src.tolist(), tgt.tolist(), w.tolist()):
            yield self.nodes[i], self.nodes[j], x

    def neighbors(self, name):
        """The names ``SymMatrix.nearest_neighbors(name, threshold)`` gives on the dense matrix, in its order: closest first,
        equally close ones in node order."""
        if self._slot is None:
            self._slot = {node: k for k, node in enumerate(self.nodes)}
        if name not in self._slot:
            raise KeyError(f"node '{name}' not in matrix")
        if self._incident is None:                               # every edge from both ends, grouped by node, the other end ascending
            node = np.concatenate([self.source, self.target])
            other = np.concatenate([self.target, self.source])
            order = np.lexsort((other, node))
            node = node[order]
            self._incident = (np.searchsorted(node, np.arange(len(self.nodes) + 1)), other[order], np.concatenate([self.weight, self.weight])[order])
        starts, other, w = self._incident
        k = self._slot[name]
        other, w = other[starts[k]:starts[k + 1]], w[starts[k]:starts[k + 1]]
        ranked = other[np.argsort(w if self.is_distance else -w, kind="stable")]
        return [self.nodes[j] for j in ranked]

    def nearest(self, k):
        """K-nearest lists of this edge list, every edge a candidate of both its ends: ``(indices, weights, count)`` -- int32[N, kk],
        float64[N, kk], int32[N], ``kk = min(k, N - 1)``.  ``count[g]`` is the number of edges that touch node g; row g lists the
        best ``min(kk, count[g])`` of them in the total order of ``NearestNeighbors`` (the better weight first, equal weights in node
        order), and the slots behind them hold ``-1`` and NaN.  A list that holds every pair gives ``NearestNeighbors.from_dense``.
        Host arithmetic (one ``np.lexsort`` over the 2 E directed edges): the statement ``Context.nearest_of_pairs`` is held to, and
        the CPU route of a held list."""
        if isinstance(k, bool) or int(k) < 1:
            raise ValueError("k must be at least 1")
        n, e = len(self.nodes), len(self)
        kk = max(min(int(k), n - 1), 0)
        owner = np.concatenate([self.source, self.target]).astype(np.int64)
        other = np.concatenate([self.target, self.source]).astype(np.int64)
        w = np.concatenate([self.weight, self.weight])
        order = np.lexsort((other, w if self.is_distance else -w, owner))
        owner, other, w = owner[order], other[order], w[order]
        count = np.bincount(owner, minlength=n).astype(np.int32) if n else np.zeros(0, dtype=np.int32)
        place = np.arange(2 * e, dtype=np.int64) - np.searchsorted(owner, owner)     # an entry's place in its owner's run
        keep = place < kk
        indices = np.full((n, kk), -1, dtype=np.int32)
        weights = np.full((n, kk), np.nan, dtype=np.float64)
        indices[owner[keep], place[keep]] = other[keep]
        weights[owner[keep], place[keep]] = w[keep]
        return indices, weights, count

    def components(self, threshold=None, strict=True):
        """Connected components of the graph over ``nodes`` whose edges are this list's pairs within ``threshold`` -- ``weight <
        threshold`` on distances, ``> threshold`` on similarities; ``<=`` / ``>=`` with ``strict=False``; ``None``: every pair
        of the list -- as int32 labels, ``labels[g]`` = the smallest index of g's component.  On distances with ``strict`` these are
        the single-linkage clusters at ``eps = threshold`` (scikit-learn merges below its ``distance_threshold``, never at it).  Host
        arithmetic (``scipy.sparse.csgraph``): the statement ``Context.fill_components`` is held to."""
        keep = np.ones(len(self), dtype=bool) if threshold is None else _passes(self.weight, threshold, self.is_distance, strict)
        return _smallest_member_labels(len(self.nodes), self.source[keep], self.target[keep])

    def extended(self, nodes, rows, values):
        """This list grown to ``nodes``: the host statement of ``edges_extend``.  ``nodes`` holds this list's nodes in their order
        and, at the ascending positions ``rows``, the new ones; ``values`` is float64[len(rows), len(nodes)], ``values[i, g]`` the
        value of the pair {rows[i], g} (a rows fill; any callable's values on the host).  The result is the stored list re-indexed
        -- the map from old to new positions is strictly increasing, so every edge keeps source < target and the list its order --
        merged with the new pairs within the threshold: ``SparseEdges.from_dense`` of the grown matrix, element for element."""
        if self.threshold is None:
            raise ValueError("SparseEdges.extended: this list carries no threshold, so which new pairs belong to it is undefined")
        old_at, rows = _grown_positions(self.nodes, nodes, rows, "SparseEdges.extended")
        src, tgt, w = _live_row_pairs(len(nodes), rows, values)
        keep = _passes(w, self.threshold, self.is_distance)
        src = np.concatenate([old_at[self.source], src[keep]])
        tgt = np.concatenate([old_at[self.target], tgt[keep]])
        w = np.concatenate([self.weight, w[keep]])
        order = np.lexsort((src, tgt))
        return SparseEdges(nodes, src[order], tgt[order], w[order], is_distance=self.is_distance, threshold=self.threshold)

    def without(self, names):
        """This list without the genomes ``names``: their edges dropped, the others re-indexed.  Exact: it is the list a fill of the
        remaining genomes delivers (a pair's value and the order depend on nothing but its two genomes and their relative order)."""
        keep_at, new_at = _positions_without(self.nodes, names, "SparseEdges.without")
        keep = (new_at[self.source] >= 0) & (new_at[self.target] >= 0)
        return SparseEdges([self.nodes[k] for k in keep_at.tolist()], new_at[self.source[keep]], new_at[self.target[keep]], self.weight[keep],
                           is_distance=self.is_distance, threshold=self.threshold)

    def rescored(self, genomes, func, as_distance=None):
        """The same edges in the same order with their weights from another metric: ``func`` over every listed pair, each with its
        ``source`` node as the reference's source, by ONE pair-list fill (``pairs_de_novo``).  ``genomes`` must hold every node of the
        list (``KeyError`` otherwise; it may hold more); with the nodes in the genomes' relative order -- as every list a fill
        delivers has them -- the weights are the cells of ``matrix_de_novo(genomes, func, ...)``.  ``as_distance``: the direction of
        the new weights (``None``: the list's own).  The result carries no threshold: what passed under one metric is no threshold
        set under another."""
        from phamclust_amd.results.pairs import pairs_de_novo
        as_distance = self.is_distance if as_distance is None else bool(as_distance)
        index = {g.name: k for k, g in enumerate(genomes)}
        stranger = next((node for node in self.nodes if node not in index), None)
        if stranger is not None:
            raise KeyError(f"SparseEdges.rescored: node '{stranger}' is not among the genomes")
        at = np.fromiter((index[node] for node in self.nodes), dtype=np.int64, count=len(self.nodes))
        pairs = np.stack([at[self.source], at[self.target]], axis=1) if len(self) else np.empty((0, 2), dtype=np.int64)
        weight = pairs_de_novo(genomes, func, pairs, as_distance=as_distance)
        return SparseEdges(self.nodes, self.source, self.target, weight, is_distance=as_distance, threshold=None)

    def inverted(self):
        """distance <-> similarity: every weight becomes round(1 - w, 6), as ``SymMatrix.invert`` does (matrix.py:236-247)."""
        return SparseEdges(self.nodes, self.source, self.target, np.round(1.0 - self.weight, 6), is_distance=not self.is_distance,
                           threshold=None if self.threshold is None else round(1.0 - self.threshold, 6))

    def to_symmatrix(self, fill):
        """The dense ``SymMatrix`` over ``nodes``: the edges' weights, ``fill`` for every absent pair, the diagonal preset."""
        n = len(self.nodes)
        data = np.full((n, n), float(fill), dtype=np.float64)
        data[self.source, self.target] = self.weight
        data[self.target, self.source] = self.weight
        np.fill_diagonal(data, 0.0 if self.is_distance else 1.0)
        return _square_matrix(self.nodes, data, self.is_distance)


PREFILTER_SLACK = 2e-6      # how far below the request the af candidates of a prefiltered peq edge list are taken (see edges_de_novo)


def _prefiltered_peq_edges(ctx, threshold, as_distance, slab_bytes):
    """The peq edge list within ``threshold`` behind its af bound, on an uploaded context: ``(src, tgt, val, stats)``.

    peq = round(round(af, 6) * round(aai, 6), 6) (metrics.py:247-253) and round(aai, 6) <= 1.0, so a pair's delivered peq similarity
    never exceeds its delivered af similarity ``a``, and its delivered peq distance is never below round(1 - a, 6).  A pair that passes
    a similarity request ``sim >= threshold`` therefore has ``a >= threshold``; one that passes a distance request ``d <= threshold``
    has round(1 - a, 6) <= threshold, so ``a >= 1 - threshold - 0.5e-6``.  The candidates are the af SIMILARITY edges at the request's
    similarity bound less ``PREFILTER_SLACK`` (four times the half-millionth of the rounding, and far above the error of the
    subtraction): a superset of every passing pair, in the edge list's own order.  The peq values of the candidates alone come from
    one pair-list fill, and the request's own predicate over those delivered values cuts the list: the plain fill's, element for
    element."""
    bound = ((1.0 - threshold) if as_distance else threshold) - PREFILTER_SLACK
    c_src, c_tgt, _, af_stats = ctx.fill_edges("af", bound, as_distance=False, slab_bytes=slab_bytes, want_stats=True, borrow=True)
    src, tgt = np.array(c_src, dtype=np.int32), np.array(c_tgt, dtype=np.int32)       # out of the loan before the next call
    val, stats = ctx.fill_pairs("peq", src, tgt, as_distance=as_distance, want_stats=True)
    keep = _passes(val, threshold, as_distance)
    stats.update(n_edges=int(keep.sum()), n_slabs=int(af_stats["n_slabs"]), n_candidates=int(src.shape[0]), af_ms_total=float(af_stats["ms_total"]),
                 af_ms_d2h=float(af_stats.get("ms_d2h", 0.0)))
    return src[keep], tgt[keep], val[keep], stats


def edges_de_novo(genomes, func, threshold, as_distance=True, slab_bytes=0, prefilter=False):
    """The edges of ``matrix_de_novo(genomes, func, cpus, as_distance)`` within ``threshold`` as a :class:`SparseEdges`, filled
    on the GPU by ``Context.fill_edges``: the dense matrix is never delivered, and beyond ``slab_bytes`` of HBM (0: automatic)
    never held.  ``func`` must be one of the six ``METRICS`` callables: there is no CPU route for this call (a generic callable
    has ``matrix_de_novo`` and ``SparseEdges.from_dense``).  With ``PHAMCLUST_GPUS`` / ``PHAMCLUST_GPU_IDS`` naming more than one
    device the fill is spread over them from this process (``MultiContext.fill_edges``: a contiguous stretch of targets per device,
    the same edges); under a launcher (``WORLD_SIZE`` > 1) it raises.

    ``prefilter=True`` (peq only; any other metric raises ``ValueError`` before any GPU call): the same list, element for element,
    in three steps on one GPU -- the af edge list at a bound no passing pair can miss (``_prefiltered_peq_edges`` has the proof),
    the peq values of those candidates alone by a pair-list fill, the request's predicate over them -- so no pair outside the af
    list is ever aligned.  What it saves depends on the threshold: much at a tight one, little at the clustering threshold."""
    if prefilter:
        from phamclust_amd.routes import _metric_name
        if _metric_name(func) != "peq":
            raise ValueError("edges_de_novo: prefilter=True is the af bound of peq and serves no other metric "
                             f"(func is {_metric_name(func) or 'no METRICS callable'})")
        names, (src, tgt, val) = _de_novo_route(genomes, func, "edges_de_novo",
            lambda ctx, metric: _prefiltered_peq_edges(ctx, threshold, as_distance, slab_bytes),
            lambda stats, record, fill_s: (
                f"{len(genomes)} genomes -> {stats['n_edges']} of {stats['n_candidates']} af candidates of {record['genome_pairs']} edges on one "
                f"device: af edges + peq pairs + D2H {fill_s:.3f} s (peq kernels {stats['ms_total']:.3f} ms, {stats['n_alignments']} alignments)"),
            several=False)
        return SparseEdges(names, src, tgt, val, is_distance=as_distance, threshold=threshold)
    names, (src, tgt, val) = _de_novo_route(genomes, func, "edges_de_novo",
        lambda ctx, metric: ctx.fill_edges(metric, threshold, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: (
            f"{len(genomes)} genomes -> {stats['n_edges']} of {record['genome_pairs']} edges in {stats['n_slabs']} slab(s) on {record['n_gpus']} "
            f"device(s): fill+compact+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)"),
        advice="for another callable: SparseEdges.from_dense(matrix_de_novo(...), threshold)")
    return SparseEdges(names, src, tgt, val, is_distance=as_distance, threshold=threshold)


def _guard_edges(names, metric, checked, values, src, tgt, weight, what):
    """Every stored edge (positions among the genomes) that touches a verified genome must carry exactly the refilled value."""
    for i, q in enumerate(checked):
        for mine, other in ((src, tgt), (tgt, src)):
            at = np.flatnonzero(mine == q)
            bad = at[weight[at] != values[i, other[at]]]
            if bad.shape[0]:
                e = int(bad[0])
                raise ValueError(f"pair ({names[int(src[e])]}, {names[int(tgt[e])]}): the {what} holds {float(weight[e])!r}, the {metric} fill gives "
                                 f"{float(values[i, int(other[e])])!r}: it was not filled with this metric from these genomes in this order")


def merge_edge_lists(first, second):
    """Two edge lists ``(source, target, weight)``, each sorted by (target, source) and sharing no pair, as one list in that order: the
    second's places among the first's by one binary search per edge, no sort."""
    (s1, t1, w1), (s2, t2, w2) = first, second
    key1 = (np.asarray(t1, dtype=np.int64) << 32) | np.asarray(s1, dtype=np.int64)
    key2 = (np.asarray(t2, dtype=np.int64) << 32) | np.asarray(s2, dtype=np.int64)
    n = key1.shape[0] + key2.shape[0]
    from_second = np.zeros(n, dtype=bool)
    from_second[np.searchsorted(key1, key2) + np.arange(key2.shape[0])] = True
    out = []
    for x1, x2, dtype in ((s1, s2, np.int32), (t1, t2, np.int32), (w1, w2, np.float64)):
        merged = np.empty(n, dtype=dtype)
        merged[from_second] = x2
        merged[~from_second] = x1
        out.append(merged)
    return tuple(out)


def edges_extend(edges, genomes, func, verify=4, slab_bytes=0):
    """New genomes against a stored edge list: the :class:`SparseEdges` over all of ``genomes`` that ``edges_de_novo(genomes, func,
    edges.threshold, edges.is_distance)`` would return, element for element, computing only the pairs that touch a genome ``edges``
    lacks (``Context.fill_rows_edges``: k new genomes cost k N pairs).  ``edges.nodes`` are a subset of the genomes' names, in the
    genomes' relative order (else ``ValueError``: orientation and tie order follow the order); a stored node that is no genome raises
    ``KeyError``; ``edges.threshold`` must be set.  ``verify`` old genomes (``matrix_extend``'s spread rule) are refilled first: every
    stored edge that touches one must carry exactly the refilled value, and every refilled pair of one with an old genome that passes
    the threshold must be stored -- a mismatch raises ``ValueError`` naming the pair; ``verify=0`` switches the guard off.  Nothing new:
    the list re-laid on the genomes' names.  Every genome new: ``edges_de_novo``.  One GPU; a callable outside ``METRICS`` and a
    launcher (``WORLD_SIZE`` > 1) raise before any GPU call (``SparseEdges.extended`` serves another callable)."""
    if edges.threshold is None:
        raise ValueError("edges_extend: the stored list carries no threshold, so which new pairs belong to it is undefined")
    plan = names, old_at, new_idx = _extend_plan(edges.nodes, genomes, "edges_extend")
    as_distance, threshold = edges.is_distance, edges.threshold
    if old_at.shape[0] == 0:
        return edges_de_novo(genomes, func, threshold, as_distance=as_distance, slab_bytes=slab_bytes)
    src, tgt, weight = old_at[edges.source], old_at[edges.target], edges.weight
    if not new_idx:
        return SparseEdges(names, src, tgt, weight, is_distance=as_distance, threshold=threshold)

    def guard(metric, checked, values):
        _guard_edges(names, metric, checked, values, src, tgt, weight, "edge list")
        stored = set(zip(src.tolist(), tgt.tolist()))
        for i, q in enumerate(checked):
            w = values[i, old_at]
            for g in old_at[_passes(w, threshold, as_distance)].tolist():
                if g != q and (min(q, g), max(q, g)) not in stored:
                    raise ValueError(f"pair ({names[min(q, g)]}, {names[max(q, g)]}): the {metric} fill gives {float(values[i, g])!r}, within the threshold "
                                     f"{threshold!r}, and the edge list lacks it: it was not filled with this metric from these genomes in this order")

    def fill(ctx, metric):
        n_src, n_tgt, n_val, stats = ctx.fill_rows_edges(metric, threshold, new_idx, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
        return (*merge_edge_lists((src, tgt, weight), (n_src, n_tgt, n_val)), stats)

    src, tgt, weight = _extend_fill(plan, genomes, func, "edges_extend", as_distance, verify, guard, fill,
        lambda stats, record, fill_s: f"{len(new_idx)} new of {len(names)} genomes -> {stats['n_pairs']} pairs, {stats['n_edges']} new edges in "
                                      f"{stats['n_slabs']} slab(s): guard+fill+compact+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)")
    return SparseEdges(names, src, tgt, weight, is_distance=as_distance, threshold=threshold)
