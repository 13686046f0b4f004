"""The nearest neighbours: each genome's k closest, without the dense matrix.

Owns ``NearestNeighbors``, its routes ``neighbors_de_novo`` and ``neighbors_extend`` with their guard (``_guard_neighbors``),
and its file (``nearest_to_file`` / ``nearest_from_file``)."""

import numpy as np

from phamclust_amd.routes import _de_novo_route, _extend_fill, _extend_plan
from phamclust_amd.results._common import _grown_positions, _similarity_lines, _similarity_lines_to_file
from phamclust_amd.results.edges import PREFILTER_SLACK, SparseEdges

NEAREST_MAX_K = 64     # PC_NEAREST_MAX_K of the C-ABI: the k a nearest-neighbours fill takes at most


class NearestNeighbors:
    """Each node's ``k`` nearest neighbours: ``indices[g]`` (int32[N, k], indices into ``nodes``) lists the nodes h != g best first
    -- the smallest weight on distances, the largest on similarities -- equally good ones in node order, and ``weights[g]``
    (float64[N, k]) their weights.  It is ``SymMatrix.nearest_neighbors(node, threshold)`` of the reference (matrix.py:265-296) with
    the threshold wide open, cut after ``k``, for every node at once; ``neighbors_de_novo`` fills it on the GPU without the dense
    matrix, ``from_dense`` states it on the host."""

    def __init__(self, nodes, indices, weights, is_distance=True):
        self.nodes = list(nodes)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        if self.indices.ndim != 2 or self.indices.shape != self.weights.shape or self.indices.shape[0] != len(self.nodes):
            raise ValueError("indices and weights must be two (len(nodes), k) arrays")
        self.is_distance = bool(is_distance)
        self._slot = None

    @classmethod
    def from_dense(cls, matrix, k):
        """The ``min(k, N - 1)`` nearest neighbours of every node of a filled ``SymMatrix``, in its current node order: per row
        one ``np.lexsort`` over (index, weight) -- the better weight first by a plain float compare, equal weights by index --
        cut after k.  Host arithmetic: the statement ``Context.fill_nearest`` is held to."""
        if int(k) < 1:
            raise ValueError("k must be at least 1")
        data = matrix._ordered()
        n = len(matrix)
        kk = max(min(int(k), n - 1), 0)
        indices = np.empty((n, kk), dtype=np.int32)
        weights = np.empty((n, kk), dtype=np.float64)
        for g in range(n):
            others = np.concatenate([np.arange(g), np.arange(g + 1, n)])
            row = data[g, others]
            if np.isnan(row).any():
                raise TypeError("cannot rank neighbours of a node with unset edges")
            order = np.lexsort((others, row if matrix.is_distance else -row))[:kk]
            indices[g] = others[order]
            weights[g] = row[order]
        return cls(matrix.nodes, indices, weights, is_distance=matrix.is_distance)

    @property
    def k(self):
        return int(self.indices.shape[1])

    def __len__(self):
        return len(self.nodes)

    def _row(self, name):
        if self._slot is None:
            self._slot = {node: g for g, node in enumerate(self.nodes)}
        if name not in self._slot:
            raise KeyError(f"node '{name}' not in matrix")
        return self._slot[name]

    def neighbors(self, name):
        """The names of ``name``'s neighbours, nearest first."""
        return [self.nodes[h] for h in self.indices[self._row(name)].tolist()]

    def weights_of(self, name):
        """Their weights, in the same order."""
        return self.weights[self._row(name)].tolist()

    def __iter__(self):
        for g, source in enumerate(self.nodes):
            for h, w in zip(self.indices[g].tolist(), self.weights[g].tolist()):
                yield source, self.nodes[h], w

    def inverted(self):
        """distance <-> similarity: every weight becomes round(1 - w, 6), as ``SparseEdges.inverted``; the order is kept."""
        return NearestNeighbors(self.nodes, self.indices, np.round(1.0 - self.weights, 6), is_distance=not self.is_distance)

    def to_edges(self, mutual=False):
        """The undirected k-nearest-neighbours graph as a :class:`SparseEdges`: the pair {g, h} is an edge when either end lists
        the other -- with ``mutual`` when both do -- once each, sorted by target, then source."""
        n, k = len(self.nodes), self.k
        g = np.repeat(np.arange(n, dtype=np.int64), k)
        h = self.indices.reshape(-1).astype(np.int64)
        pair = np.maximum(g, h) * n + np.minimum(g, h)                   # ascending = by target, then source
        pair, first, listed = np.unique(pair, return_index=True, return_counts=True)
        keep = listed == 2 if mutual else np.ones(pair.shape[0], dtype=bool)
        pair, first = pair[keep], first[keep]
        return SparseEdges(self.nodes, pair % max(n, 1), pair // max(n, 1), self.weights.reshape(-1)[first], is_distance=self.is_distance)

    def extended(self, nodes, rows, values, k=None):
        """These lists grown to ``nodes``: the host statement of ``neighbors_extend`` (arguments as ``SparseEdges.extended``:
        ``values[i]`` holds the weights of node ``rows[i]`` against all of ``nodes``), equal to ``from_dense`` of the grown matrix cut
        after ``k`` (default: this result's k).  An old node's stored list is the best of its old candidates, and every old
        candidate outside it is worse than every entry in it, so the best k of {stored list} + {its pairs with the new nodes} is the
        best k of all; a new node's row holds all of its candidates.  The old nodes keep their relative order, so re-indexing
        changes no comparison.  ``k`` above this result's k is a ``ValueError`` unless the stored lists are complete (k = N_old - 1)."""
        old_at, rows = _grown_positions(self.nodes, nodes, rows, "NearestNeighbors.extended")
        n, n_old = len(nodes), len(self.nodes)
        k = self.k if k is None else int(k)
        if k > self.k and self.k < n_old - 1:
            raise ValueError(f"NearestNeighbors.extended: the stored lists hold {self.k} of {n_old - 1} old neighbours and cannot decide {k}")
        if k < 1 and n > 1:
            raise ValueError("k must be at least 1")
        kk = max(min(k, n - 1), 0)
        values = np.asarray(values, dtype=np.float64).reshape(len(rows), n)
        if np.isnan(values).any():
            raise TypeError("cannot rank neighbours of a node with unset edges")
        sign = 1.0 if self.is_distance else -1.0
        indices = np.empty((n, kk), dtype=np.int32)
        weights = np.empty((n, kk), dtype=np.float64)
        for g, at in enumerate(old_at.tolist()):
            others = np.concatenate([old_at[self.indices[g]], rows])
            row = np.concatenate([self.weights[g], values[:, at]])
            order = np.lexsort((others, sign * row))[:kk]
            indices[at], weights[at] = others[order], row[order]
        for i, q in enumerate(rows.tolist()):
            others = np.concatenate([np.arange(q), np.arange(q + 1, n)])
            row = values[i, others]
            order = np.lexsort((others, sign * row))[:kk]
            indices[q], weights[q] = others[order], row[order]
        return NearestNeighbors(nodes, indices, weights, is_distance=self.is_distance)

    def without(self, names):
        """Refused: a list that named a removed genome needs its (k+1)-th entry to stay k long, and only a fill knows it
        (``neighbors_de_novo`` over the remaining genomes)."""
        raise ValueError("NearestNeighbors.without: a list that named a removed genome needs its next-best entry, which only a fill knows; "
                         "removing genomes needs a fill of the remaining ones (neighbors_de_novo)")


NEAREST_PAIRS_MAX = 2 ** 30     # pairs one Context.nearest_of_pairs call takes


def _bounded_peq_nearest(ctx, k, as_distance, slab_bytes):
    """The peq k-nearest lists behind their af bound, on an uploaded context: ``(nbr, val, stats)``, the lists of
    ``ctx.fill_nearest("peq", k)`` element for element.  ``kk = min(k, N - 1)``; "better" and the total order are the fill's.

    peq = round(round(af, 6) * round(aai, 6), 6) (metrics.py:247-253) and round(aai, 6) <= 1.0, so a pair's delivered peq similarity
    never exceeds its delivered af similarity ``a``, and its delivered peq distance is never below round(1 - a, 6)
    (``_prefiltered_peq_edges``).  The nearest fill has no threshold to hold that against; it has one per genome:

    1. Seed.  ``fill_nearest("af", kk)`` as similarities; the seed pairs are every {g, h} with h in g's af list, oriented
       source < target, each once: at most N kk pairs.
    2. Bars.  The peq values of the seed pairs (one pair-list fill) become k-nearest lists (``nearest_of_pairs``: a pair is a
       candidate of both its ends).  Every genome has at least kk entries -- its own af list holds kk pairs that contain it -- and
       ``bar[g]`` is the kk-th value of g's list.  The list is made of true pairs of g, so g's true kk-th best is as good or better.
    3. Candidates.  Any h in g's true top kk has a delivered peq value at least as good as ``bar[g]``.  On similarities
       peq <= a, so ``a >= bar[g]``; on distances d_peq >= round(1 - a, 6), so round(1 - a, 6) <= bar[g] and
       ``a >= (1 - bar[g]) - PREFILTER_SLACK`` (the slack covers the half-millionth of the rounding and the subtraction's error, as
       for the edge list; the delivered af DISTANCE is no bound, it can lie a millionth above round(1 - a, 6)).  The candidates are
       the pairs (s < t) whose af similarity reaches ``simbar[s]`` or ``simbar[t]`` -- non-strictly, since equal values order by
       index -- which is ``fill_edges_bars("af", simbar)``: they contain every true top-kk pair of every genome.
    4. Result.  The peq values of the candidates (one pair-list fill), then ``nearest_of_pairs`` over that list ALONE: each genome's
       true top kk are all in it and everything else in it is a true pair that ranks behind them, so the best kk of the list are the
       best kk of all, in the same total order.  The seed pairs are not merged in (most are candidates again; one list holds no pair
       twice).
    5. Fallback.  More candidates than half the triangle (or than one ``nearest_of_pairs`` call takes): they are dropped and the plain
       ``fill_nearest("peq", k)`` runs -- the same result by definition.

    ``stats``: the last peq call's, with ``k``, ``n_slabs`` (the candidate pass's, or the plain fill's), ``n_seed_pairs``,
    ``n_candidates``, ``n_alignments`` (every peq call of the route), ``fallback``, ``af_ms_total`` (both af fills), ``af_ms_d2h`` (the candidates' copy to the host), ``ms_total`` (every
    fill of the route), ``n_list_bytes`` (what the pair lists moved over PCIe: 16 bytes per edge down, 8 up and 8 down per pair value, 16 up per listed pair) and ``step_s`` (host seconds of the seed af
    fill, the seed peq values, the seed lists, the candidate pass, the final peq values, the final lists or the fallback)."""
    import time
    n = ctx.n_genomes
    total = n * (n - 1) // 2
    kk = max(min(int(k), n - 1), 0)
    route = dict(n_seed_pairs=0, n_candidates=0, fallback=0, af_ms_total=0.0, af_ms_d2h=0.0, n_list_bytes=0)
    if kk == 0:                                                         # (N == 1: nothing to bound)
        nbr, val, stats = ctx.fill_nearest("peq", int(k), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
        return nbr, val, dict(stats, **route, step_s=[0.0] * 6)
    clock = [time.perf_counter()]
    a_nbr, _, af_stats = ctx.fill_nearest("af", kk, as_distance=False, slab_bytes=slab_bytes, want_stats=True)
    g, h = np.repeat(np.arange(n, dtype=np.int64), kk), np.asarray(a_nbr, dtype=np.int64).reshape(-1)
    pair = np.unique(np.maximum(g, h) * n + np.minimum(g, h))
    s_src, s_tgt = (pair % n).astype(np.int32), (pair // n).astype(np.int32)
    clock.append(time.perf_counter())
    s_val, seed_stats = ctx.fill_pairs("peq", s_src, s_tgt, as_distance=as_distance, want_stats=True)
    clock.append(time.perf_counter())
    _, l_val, l_count = ctx.nearest_of_pairs(s_src, s_tgt, s_val, kk, as_distance=as_distance)
    if int(l_count.min()) < kk:
        raise RuntimeError(f"bounded nearest fill: a genome has {int(l_count.min())} seed pairs, below k = {kk}: the af lists are not what fill_nearest delivers")
    bar = np.ascontiguousarray(l_val[:, kk - 1])
    simbar = ((1.0 - bar) - PREFILTER_SLACK) if as_distance else bar
    clock.append(time.perf_counter())
    c_src, c_tgt, _, cand_stats = ctx.fill_edges_bars("af", simbar, as_distance=False, slab_bytes=slab_bytes, want_stats=True)
    clock.append(time.perf_counter())
    n_cand = int(c_src.shape[0])
    route.update(n_seed_pairs=int(pair.shape[0]), n_candidates=n_cand, af_ms_total=float(af_stats["ms_total"]) + float(cand_stats["ms_total"]),
                 af_ms_d2h=float(cand_stats.get("ms_d2h", 0.0)), n_list_bytes=int(pair.shape[0]) * 32 + n_cand * 16)
    if 2 * n_cand > total or n_cand > NEAREST_PAIRS_MAX:
        nbr, val, stats = ctx.fill_nearest("peq", int(k), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
        clock += [clock[-1], time.perf_counter()]
        route.update(fallback=1)
    else:
        c_val, stats = ctx.fill_pairs("peq", c_src, c_tgt, as_distance=as_distance, want_stats=True)
        clock.append(time.perf_counter())
        nbr, val, count = ctx.nearest_of_pairs(c_src, c_tgt, c_val, kk, as_distance=as_distance)
        clock.append(time.perf_counter())
        if int(count.min()) < kk:
            raise RuntimeError(f"bounded nearest fill: a genome has {int(count.min())} candidates, below k = {kk}: the af bound does not hold on this collection")
        route.update(n_list_bytes=route["n_list_bytes"] + n_cand * 32)
        stats = dict(stats, k=kk, n_slabs=int(cand_stats["n_slabs"]))
    stats = dict(stats, **route, n_alignments=int(stats["n_alignments"]) + int(seed_stats["n_alignments"]),
                 ms_total=float(stats["ms_total"]) + float(seed_stats["ms_total"]) + route["af_ms_total"],
                 step_s=[b - a for a, b in zip(clock, clock[1:])])
    return nbr, val, stats


def neighbors_de_novo(genomes, func, k, as_distance=True, slab_bytes=0, bound=False):
    """Each genome's ``k`` nearest neighbours in ``matrix_de_novo(genomes, func, cpus, as_distance)`` as a
    :class:`NearestNeighbors`, filled on the GPU by ``Context.fill_nearest``: the dense matrix is never delivered, and beyond
    ``slab_bytes`` of HBM (0: automatic) never held; N * k entries cross PCIe.  ``func`` must be one of the six ``METRICS``
    callables (no CPU route: ``NearestNeighbors.from_dense(matrix_de_novo(...), k)`` serves another callable).  Several devices as
    ``edges_de_novo`` (``MultiContext.fill_nearest``: the same lists); under a launcher (``WORLD_SIZE`` > 1) it raises.  Every
    refusal comes before the first GPU call.

    ``bound=True`` (peq only; any other metric raises ``ValueError`` before any GPU call): the same lists, element for element, on one
    GPU behind the af bound of peq -- each genome's own k-th best value so far is its bar, and only pairs whose af similarity can
    reach the bar of either end are aligned (``_bounded_peq_nearest`` has the rule and its proof).  What it saves depends on the
    collection and on k; when more than half the pairs stay candidates it falls back to the plain fill."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= NEAREST_MAX_K:
        raise ValueError(f"neighbors_de_novo: k must be an integer in 1..{NEAREST_MAX_K}, not {k!r}")
    if bound:
        from phamclust_amd.routes import _metric_name
        if _metric_name(func) != "peq":
            raise ValueError("neighbors_de_novo: bound=True is the af bound of peq and serves no other metric "
                             f"(func is {_metric_name(func) or 'no METRICS callable'})")
        names, (nbr, val) = _de_novo_route(genomes, func, "neighbors_de_novo",
            lambda ctx, metric: _bounded_peq_nearest(ctx, int(k), as_distance, slab_bytes),
            lambda stats, record, fill_s: (
                f"{len(genomes)} genomes -> {stats['k']} nearest neighbours each from {stats['n_candidates']} af candidates of {record['genome_pairs']} "
                f"pairs on one device ({stats['n_seed_pairs']} seed pairs{', fell back to the plain fill' if stats['fallback'] else ''}): "
                f"af fills + peq pairs + select + D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, {stats['n_alignments']} alignments)"),
            several=False)
        return NearestNeighbors(names, nbr, val, is_distance=as_distance)
    names, (nbr, val) = _de_novo_route(genomes, func, "neighbors_de_novo",
        lambda ctx, metric: ctx.fill_nearest(metric, int(k), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: f"{len(genomes)} genomes -> {stats['k']} nearest neighbours each from {record['genome_pairs']} pairs in "
                                      f"{stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): fill+select+D2H {fill_s:.3f} s (kernels "
                                      f"{stats['ms_total']:.3f} ms, selection {stats.get('ms_select', 0.0):.3f} ms)")
    return NearestNeighbors(names, nbr, val, is_distance=as_distance)


def _guard_neighbors(names, metric, checked, values, old_at, indices, weights, is_distance):
    """For every verified old genome (``checked``: positions among the genomes; ``values``: their refilled rows) the best of its
    refilled row, restricted to the old genomes, must equal its stored list -- ``indices`` (positions among the genomes) and
    ``weights`` [N_old, k] -- in indices and value bits."""
    k = indices.shape[1]
    slot = {int(g): i for i, g in enumerate(old_at.tolist())}
    for i, q in enumerate(checked):
        others = old_at[old_at != q]
        row = np.ascontiguousarray(values[i, others], dtype=np.float64)
        order = np.lexsort((others, row if is_distance else -row))[:k]
        want_idx, want_w = others[order], row[order]
        have_idx, have_w = indices[slot[q]], np.ascontiguousarray(weights[slot[q]], dtype=np.float64)
        bad = np.flatnonzero((want_idx != have_idx) | (want_w.view(np.uint64) != have_w.view(np.uint64)))
        if bad.shape[0]:
            j = int(bad[0])
            raise ValueError(f"pair ({names[q]}, {names[int(have_idx[j])]}): the nearest-neighbours list holds it at place {j + 1} with {float(have_w[j])!r}, the "
                             f"{metric} fill gives ({names[int(want_idx[j])]}, {float(want_w[j])!r}) there: it was not filled with this metric from these "
                             f"genomes in this order")


def neighbors_extend(neighbors, genomes, func, k=None, verify=4, slab_bytes=0):
    """New genomes against stored k-nearest lists: the :class:`NearestNeighbors` over all of ``genomes`` that
    ``neighbors_de_novo(genomes, func, k, neighbors.is_distance)`` would return, element for element, computing only the pairs that
    touch a genome ``neighbors`` lacks (``Context.fill_rows_nearest``: the stored lists seed the resident ones).  ``k`` defaults to
    ``neighbors.k``; ``k > neighbors.k`` is a ``ValueError`` unless the stored lists are complete (``neighbors.k == N_old - 1``): a
    shorter list cannot decide more neighbours.  Arguments, refusals and routes as ``tree_extend``.  The guard: for each verified old
    genome, the best ``neighbors.k`` of its refilled row, restricted to the old genomes, must equal its stored list in indices and
    value bits.  Removing genomes is no such call: ``NearestNeighbors.without`` says why."""
    plan = names, old_at, new_idx = _extend_plan(neighbors.nodes, genomes, "neighbors_extend")
    as_distance, n_old = neighbors.is_distance, int(old_at.shape[0])
    if k is None:
        k = neighbors.k
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= NEAREST_MAX_K:
        raise ValueError(f"neighbors_extend: k must be an integer in 1..{NEAREST_MAX_K}, not {k!r}")
    k = int(k)
    if n_old and k > neighbors.k and neighbors.k < n_old - 1:
        raise ValueError(f"neighbors_extend: the stored lists hold {neighbors.k} of {n_old - 1} old neighbours and cannot decide {k}: fill from scratch "
                         "(neighbors_de_novo)")
    if n_old == 0:
        return neighbors_de_novo(genomes, func, k, as_distance=as_distance, slab_bytes=slab_bytes)
    indices = old_at[neighbors.indices].reshape(n_old, neighbors.k)
    if not new_idx:
        return NearestNeighbors(names, indices[:, :min(k, neighbors.k)], neighbors.weights[:, :min(k, neighbors.k)], is_distance=as_distance)

    def fill(ctx, metric):
        seed_nbr = np.zeros((len(names), neighbors.k), dtype=np.int32)
        seed_val = np.zeros((len(names), neighbors.k), dtype=np.float64)
        seed_nbr[old_at], seed_val[old_at] = indices, neighbors.weights
        return ctx.fill_rows_nearest(metric, k, new_idx, seed=(seed_nbr, seed_val), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)

    nbr, val = _extend_fill(plan, genomes, func, "neighbors_extend", as_distance, verify,
        lambda metric, checked, values: _guard_neighbors(names, metric, checked, values, old_at, indices, neighbors.weights, as_distance), fill,
        lambda stats, record, fill_s: (
            f"{len(new_idx)} new of {len(names)} genomes -> {stats['n_pairs']} pairs, the {stats['k']} nearest of each in {stats['n_slabs']} slab(s): "
            f"guard+fill+select+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, selection {stats.get('ms_select', 0.0):.3f} ms)"))
    return NearestNeighbors(names, nbr, val, is_distance=as_distance)


def nearest_to_file(found, filepath):
    """``nearest_<metric>.tsv``: one ``source<TAB>target<TAB>similarity`` line per neighbour of a distance result, sources in node
    order, targets nearest first; the weights inverted as for the adjacency file, "%.6f"."""
    return _similarity_lines_to_file(found, filepath)


def nearest_from_file(filepath, names):
    """The distance :class:`NearestNeighbors` a ``nearest_<metric>.tsv`` holds, bit for bit: its nodes are the names that occur as
    sources in the file, in the order of ``names`` (the genomes in fill order; ``KeyError`` for a name they lack), and a similarity
    comes back as ``tree_from_file`` decodes it.  ``ValueError`` for a line that is no neighbour, sources whose lines are not together
    or come in another order than ``names``, an unequal number of lines per source, a count other than min(K, n - 1) (more than
    n - 1 lines for n sources, or none), or a target that is no source, the source itself, or listed twice."""
    index = {name: k for k, name in enumerate(names)}
    sources, lists = [], []
    for number, s, t, k in _similarity_lines(filepath, index):
        if not sources or sources[-1] != s:
            if sources and s <= sources[-1]:
                raise ValueError(f"{filepath}:{number}: source '{names[s]}' comes against the genomes' order (or its lines are not together): "
                                 "the file was written for another order")
            sources.append(s)
            lists.append([])
        lists[-1].append((t, (1000000 - k) / 1000000.0))
    n = len(sources)
    count = len(lists[0]) if lists else 0
    uneven = next((g for g, one in zip(sources, lists) if len(one) != count), None)
    if uneven is not None:
        raise ValueError(f"{filepath}: '{names[uneven]}' has {len(lists[sources.index(uneven)])} lines, '{names[sources[0]]}' has {count}: every source "
                         "lists the same number of neighbours")
    if n and not 1 <= count <= n - 1:
        raise ValueError(f"{filepath}: {count} neighbours per source for {n} sources is no min(K, n - 1)")
    at = {g: k for k, g in enumerate(sources)}
    for g, one in zip(sources, lists):
        targets = [t for t, _ in one]
        bad = next((t for t in targets if t not in at or t == g), None)
        if bad is not None or len(set(targets)) != len(targets):
            raise ValueError(f"{filepath}: the neighbours of '{names[g]}' must be distinct other sources of the file"
                             + (f" ('{names[bad]}' is not)" if bad is not None else ""))
    indices = np.asarray([[at[t] for t, _ in one] for one in lists], dtype=np.int32).reshape(n, count)
    weights = np.asarray([[w for _, w in one] for one in lists], dtype=np.float64).reshape(n, count)
    return NearestNeighbors([names[g] for g in sources], indices, weights, is_distance=True)
