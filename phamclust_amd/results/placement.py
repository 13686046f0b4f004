"""The placement: new genomes against the groups of a stored partition -- for every query genome the sum, minimum and maximum to every
group, its own entry and the nearest other group by three criteria, and what the queries add to the old genomes' own entries --
without the dense matrix and without refilling the pairs among the old genomes.

Owns ``GroupPlacement``, its route ``placement_de_novo`` and its file (``placement_to_file`` / ``placement_from_file``)."""

import numpy as np

from phamclust_amd.routes import _de_novo_route, _group_indices, _name_index
from phamclust_amd.results.affinity import AFFINITY_KINDS, GroupAffinity
from phamclust_amd.results.linkage import BETWEEN_MAX_GROUPS, MILLION, _EMPTY_HI, _EMPTY_LO


def _placement_labels(nodes, at, groups, who):
    """int32 ``label[g]`` = the group of node g or -1: in no group.  KeyError for a member that is no node, ValueError for a node in two groups."""
    label = np.full(len(nodes), -1, dtype=np.int32)
    for b, group in enumerate(groups):
        for name in group:
            if name not in at:
                raise KeyError(f"{who}: '{name}' of group {b} is no node")
            if label[at[name]] >= 0:
                raise ValueError(f"{who}: '{name}' is in two groups")
            label[at[name]] = b
    return label


def _flipped(total, lo, hi, count):
    """distance <-> similarity of (sum, lo, hi) entries counting ``count`` pairs; empty entries stay empty."""
    full = count > 0
    return (np.where(full, count * MILLION - total, 0), np.where(full, MILLION - np.asarray(hi, dtype=np.int64), _EMPTY_LO),
            np.where(full, MILLION - np.asarray(lo, dtype=np.int64), _EMPTY_HI))


class GrownOwn:
    """The own entries of a partition after the queries joined it: ``own_sum`` (int64), ``own_lo``, ``own_hi`` (int32) over ``nodes``
    -- what ``GroupAffinity`` of the whole collection holds under these names (a node in no group: empty) -- and the medoids read
    from them."""

    def __init__(self, nodes, groups, own_sum, own_lo, own_hi, is_distance):
        self.nodes, self.groups = list(nodes), [list(group) for group in groups]
        self.own_sum = np.ascontiguousarray(own_sum, dtype=np.int64)
        self.own_lo = np.ascontiguousarray(own_lo, dtype=np.int32)
        self.own_hi = np.ascontiguousarray(own_hi, dtype=np.int32)
        self.is_distance = bool(is_distance)
        self._at = {name: k for k, name in enumerate(self.nodes)}

    def medoids(self):
        """Per group its medoid's name (None for an empty group), by ``GroupAffinity.medoids``' rule."""
        out = []
        for group in self.groups:
            if not group:
                out.append(None)
                continue
            sums = self.own_sum[[self._at[name] for name in group]]
            out.append(group[int(np.argmin(sums) if self.is_distance else np.argmax(sums))])
        return out


class GroupPlacement:
    """How the query genomes of a collection relate to the groups of a partition of it, in MILLIONTHS: what
    ``Context.fill_rows_affinity`` delivers and ``from_dense`` states on the host.  ``nodes`` are the genomes in array order, ``groups``
    lists of their names -- a node is in ONE group or in none (``label[g] == -1``); ``sizes[b]`` counts a group's members, queries
    included -- and ``queries`` the query genomes' names in array order.  Per query k (``GroupAffinity``'s statement of genome
    ``queries[k]``): ``own_sum`` (int64), ``own_lo``, ``own_hi`` (int32) -- empty for a query in no group; ``near_group`` (int32
    ``[3, n_queries]``): the non-empty group other than its own nearest by mean, by minimum and by maximum DISTANCE (ties to the smaller
    index, -1: none; a query in no group has every non-empty group for a candidate), with ``near_sum``, ``near_lo``, ``near_hi``.
    ``table``: None or ``(sum, lo, hi)`` of ``[n_queries, G]`` arrays, entry ``[k, b]`` counting ``sizes[b] - (label of query k == b)``
    pairs.  ``gain``: None or ``(sum, lo, hi)`` of ``[N]`` arrays: for a node that is no query and is in a group, its values to the
    QUERIES of its own group -- what they add to its own entry (``grown_own``); empty elsewhere.  An empty entry reads ``0, 2**31 - 1,
    -1``.  On similarities (``is_distance=False``) the groups are those of the inverted matrix and every value is the complement."""

    def __init__(self, nodes, groups, queries, own_sum, own_lo, own_hi, near_group, near_sum, near_lo, near_hi, table=None, gain=None, is_distance=True):
        self.nodes = list(nodes)
        self.groups = [list(group) for group in groups]
        self.queries = list(queries)
        n, g, k = len(self.nodes), len(self.groups), len(self.queries)
        at = {name: i for i, name in enumerate(self.nodes)}
        if len(at) != n:
            raise ValueError("GroupPlacement: node names must be distinct")
        self._at = at
        self.label = _placement_labels(self.nodes, at, self.groups, "GroupPlacement")
        stranger = next((name for name in self.queries if name not in at), None)
        if stranger is not None:
            raise KeyError(f"GroupPlacement: query '{stranger}' is no node")
        self.query_at = np.array([at[name] for name in self.queries], dtype=np.int64)
        if k > 1 and not (np.diff(self.query_at) > 0).all():
            raise ValueError("GroupPlacement: the queries must be distinct and in the nodes' order")
        self.query_label = self.label[self.query_at] if k else np.empty(0, dtype=np.int32)
        self.sizes = np.array([len(group) for group in self.groups], dtype=np.int64)
        self.own_sum = np.ascontiguousarray(own_sum, dtype=np.int64)
        self.own_lo = np.ascontiguousarray(own_lo, dtype=np.int32)
        self.own_hi = np.ascontiguousarray(own_hi, dtype=np.int32)
        self.near_group = np.ascontiguousarray(near_group, dtype=np.int32)
        self.near_sum = np.ascontiguousarray(near_sum, dtype=np.int64)
        self.near_lo = np.ascontiguousarray(near_lo, dtype=np.int32)
        self.near_hi = np.ascontiguousarray(near_hi, dtype=np.int32)
        for name in ("own_sum", "own_lo", "own_hi", "near_sum", "near_lo", "near_hi"):
            if getattr(self, name).shape != (k,):
                raise ValueError(f"GroupPlacement: {name} must hold {k} entries, not {getattr(self, name).shape}")
        if self.near_group.shape != (3, k):
            raise ValueError(f"GroupPlacement: near_group must be 3 x {k}, not {self.near_group.shape}")
        self.table = self._triple(table, (k, g), "the table")
        self.gain = self._triple(gain, (n,), "the gain")
        self.is_distance = bool(is_distance)

    @staticmethod
    def _triple(arrays, shape, what):
        if arrays is None:
            return None
        total, lo, hi = arrays
        out = (np.ascontiguousarray(total, dtype=np.int64), np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32))
        if any(arr.shape != shape for arr in out):
            raise ValueError(f"GroupPlacement: {what} must be three arrays of shape {shape}")
        return out

    def __len__(self):
        return len(self.queries)

    def _arrays(self):
        return (self.own_sum, self.own_lo, self.own_hi, self.near_group, self.near_sum, self.near_lo, self.near_hi)

    def __eq__(self, other):
        def same(a, b):
            return (a is None) == (b is None) and (a is None or all(np.array_equal(x, y) for x, y in zip(a, b)))
        return (isinstance(other, GroupPlacement) and self.nodes == other.nodes and self.groups == other.groups and self.queries == other.queries and
                self.is_distance == other.is_distance and same(self._arrays(), other._arrays()) and same(self.table, other.table) and
                same(self.gain, other.gain))

    __hash__ = None

    # -- the counts no array stores
    def _own_count(self):
        """``[n_queries]``: the other members of a query's own group; 0 for a query in no group."""
        labelled = self.query_label >= 0
        return np.where(labelled, self.sizes[np.maximum(self.query_label, 0)] - 1 if len(self.sizes) else 0, 0)

    def counts(self):
        """``[n_queries, G]``: the pairs entry ``[k, b]`` counts, ``sizes[b] - (label of query k == b)``."""
        count = np.broadcast_to(self.sizes, (len(self.queries), len(self.groups))).copy()
        mine = np.flatnonzero(self.query_label >= 0)
        count[mine, self.query_label[mine]] -= 1
        return count

    def gain_counts(self):
        """``[N]``: the pairs a gain entry counts -- the queries of the node's own group; 0 for a query and for a node in no group."""
        per_group = np.bincount(self.query_label[self.query_label >= 0], minlength=max(len(self.groups), 1)).astype(np.int64)
        count = np.where(self.label >= 0, per_group[np.maximum(self.label, 0)], 0)
        count[self.query_at] = 0
        return count

    @classmethod
    def _from_distance_table(cls, nodes, groups, queries, total, lo, hi, gain, is_distance, keep_table):
        """The per-query statement read off the DISTANCE rows (int64 ``[n_queries, G]``, empty entries in the empty convention): ``GroupAffinity``'s
        rule -- ascending groups, strictly better only -- with an own group that may be none."""
        at = {name: i for i, name in enumerate(nodes)}
        label = _placement_labels(nodes, at, groups, "GroupPlacement")
        q_label = label[[at[name] for name in queries]].astype(np.int64) if len(queries) else np.empty(0, dtype=np.int64)
        sizes = np.array([len(group) for group in groups], dtype=np.int64)
        k = len(queries)
        best = [np.full(k, -1, dtype=np.int64) for _ in range(3)]
        b_sum, b_size = np.zeros(k, dtype=np.int64), np.ones(k, dtype=np.int64)
        b_lo, b_hi = np.full(k, _EMPTY_LO, dtype=np.int64), np.full(k, _EMPTY_LO, dtype=np.int64)
        for b in range(len(groups)):
            if not sizes[b]:
                continue
            other = q_label != b                                            # (a group that holds the query alone is its own: no candidate)
            take = other & ((best[0] < 0) | (total[:, b] * b_size < b_sum * sizes[b]))
            best[0][take], b_sum[take], b_size[take] = b, total[take, b], sizes[b]
            take = other & ((best[1] < 0) | (lo[:, b] < b_lo))
            best[1][take], b_lo[take] = b, lo[take, b]
            take = other & ((best[2] < 0) | (hi[:, b] < b_hi))
            best[2][take], b_hi[take] = b, hi[take, b]
        none = best[0] < 0
        mine, rows, own = q_label >= 0, np.arange(k), np.maximum(q_label, 0)

        def pick(arr, empty):                                               # a query's entry for its own group; a query in none: empty
            return np.where(mine, arr[rows, own], empty) if len(groups) else np.full(k, empty, dtype=np.int64)
        out = cls(nodes, groups, queries, pick(total, 0), pick(lo, _EMPTY_LO), pick(hi, _EMPTY_HI), np.stack(best), np.where(none, 0, b_sum),
                  np.where(none, _EMPTY_LO, b_lo), np.where(none, _EMPTY_HI, b_hi), table=(total, lo, hi) if keep_table else None, gain=gain,
                  is_distance=True)
        return out if is_distance else out.inverted()

    @classmethod
    def from_dense(cls, matrix, groups, queries, want_table=True, want_gain=True):
        """The host statement of the definition, in integers, by numpy: the placement of ``queries`` (names of ``matrix``) against
        ``groups`` (lists of names of ``matrix``, a node in at most one) over the weights of ``matrix``, the nodes in the matrix's
        order.  Nodes that appear in no group -- queries or not -- are unlabelled: no entry counts them.  A similarity matrix gives
        the statement of its ``invert()``, inverted.  ValueError for a weight that is unset or no millionth."""
        groups = [list(group) for group in groups]
        nodes = matrix.nodes
        data = np.asarray(matrix._ordered(), dtype=np.float64)
        n, g = len(nodes), len(groups)
        micro = np.rint(data * 1.0e6)
        exact = micro / 1.0e6 == data
        np.fill_diagonal(exact, True)                                       # the diagonal: no pair
        np.fill_diagonal(micro, 0.0)
        if not (micro >= 0.0).all() or not (micro <= 1.0e6).all() or not exact.all():
            raise ValueError("GroupPlacement.from_dense: a weight is unset or no millionth in [0, 1]")
        micro = micro.astype(np.int64)
        if not matrix.is_distance:
            micro = MILLION - micro
        at = {name: i for i, name in enumerate(nodes)}
        label = _placement_labels(nodes, at, groups, "GroupPlacement.from_dense")
        stranger = next((name for name in queries if name not in at), None)
        if stranger is not None:
            raise KeyError(f"node '{stranger}' not in matrix")
        q_at = np.array(sorted(at[name] for name in queries), dtype=np.int64)
        if np.unique(q_at).shape[0] != q_at.shape[0]:
            raise ValueError("GroupPlacement.from_dense: a query is listed twice")
        queries = [nodes[i] for i in q_at]
        k = q_at.shape[0]
        total = np.zeros((k, g), dtype=np.int64)
        lo = np.full((k, g), _EMPTY_LO, dtype=np.int64)
        hi = np.full((k, g), _EMPTY_HI, dtype=np.int64)
        labelled = label >= 0
        for j, q in enumerate(q_at.tolist()):                               # entry [j][b]: over the members of b but the query itself
            cols = np.flatnonzero(labelled & (np.arange(n) != q))
            np.add.at(total[j], label[cols], micro[q, cols])
            np.minimum.at(lo[j], label[cols], micro[q, cols])
            np.maximum.at(hi[j], label[cols], micro[q, cols])
        gain = None
        if want_gain:
            is_query = np.zeros(n, dtype=bool)
            is_query[q_at] = True
            g_sum, g_lo, g_hi = np.zeros(n, dtype=np.int64), np.full(n, _EMPTY_LO, dtype=np.int64), np.full(n, _EMPTY_HI, dtype=np.int64)
            for q in q_at.tolist():
                if label[q] < 0:
                    continue
                old = np.flatnonzero((label == label[q]) & ~is_query)
                g_sum[old] += micro[old, q]
                g_lo[old] = np.minimum(g_lo[old], micro[old, q])
                g_hi[old] = np.maximum(g_hi[old], micro[old, q])
            gain = (g_sum, g_lo, g_hi)
        return cls._from_distance_table(nodes, groups, queries, total, lo, hi, gain, matrix.is_distance, want_table)

    def inverted(self):
        """distance <-> similarity: the same nearest groups, every value complemented as ``GroupAffinity.inverted`` does it -- the gain
        over ``gain_counts()``; empty entries stay empty."""
        own = _flipped(self.own_sum, self.own_lo, self.own_hi, self._own_count())
        near = self.near_group[0] >= 0
        near_size = np.where(near, self.sizes[np.maximum(self.near_group[0], 0)] if len(self.sizes) else 0, 0)
        table = None if self.table is None else _flipped(*self.table, self.counts())
        gain = None if self.gain is None else _flipped(*self.gain, self.gain_counts())
        return GroupPlacement(self.nodes, self.groups, self.queries, *own, self.near_group, np.where(near, near_size * MILLION - self.near_sum, 0),
                              np.where(near, MILLION - self.near_lo.astype(np.int64), _EMPTY_LO), np.where(near, MILLION - self.near_hi.astype(np.int64), _EMPTY_HI),
                              table=table, gain=gain, is_distance=not self.is_distance)

    @staticmethod
    def _kind(kind, who):
        if kind not in AFFINITY_KINDS:
            raise ValueError(f"GroupPlacement.{who}: kind must be 'mean', 'nearest' or 'farthest', not {kind!r}")
        return AFFINITY_KINDS.index(kind)

    def nearest_group(self, kind="mean"):
        """``[n_queries]`` int32: the non-empty group other than the query's own nearest by ``kind`` (``AFFINITY_KINDS``); -1: none."""
        return self.near_group[self._kind(kind, "nearest_group")].copy()

    def nearest_value(self, kind="mean"):
        """``[n_queries]`` float64: the value that made ``nearest_group(kind)`` nearest -- the mean value to it, the best single value, or
        the worst; ``nan`` where there is no such group."""
        k = self._kind(kind, "nearest_value")
        group = self.near_group[k]
        there = group >= 0
        out = np.full(len(self.queries), np.nan)
        if k == 0:
            out[there] = self.near_sum[there] / (self.sizes[group[there]] * float(MILLION))
        else:
            out[there] = (self.near_lo if k == 1 else self.near_hi)[there] / float(MILLION)
        return out

    def _near_similarity_micro(self, k):
        """(numerator, denominator) per query: the SIMILARITY behind ``nearest_group`` of criterion k is numerator / denominator millionths."""
        group = self.near_group[k]
        size = np.where(group >= 0, self.sizes[np.maximum(group, 0)] if len(self.sizes) else 1, 1)
        if k == 0:
            value, count = self.near_sum, size
        else:
            value, count = (self.near_lo if k == 1 else self.near_hi).astype(np.int64), np.ones_like(size)
        return (count * MILLION - value if self.is_distance else value), count

    def assigned(self, kind="mean", min_similarity=None):
        """name -> group index or None, per query: ``nearest_group(kind)``, and None where there is no group or, with ``min_similarity``
        (a fraction), where the similarity that made it nearest -- compared in integers, as millionths -- lies below it."""
        k = self._kind(kind, "assigned")
        group = self.near_group[k]
        keep = group >= 0
        if min_similarity is not None:
            value, count = self._near_similarity_micro(k)
            keep &= value >= int(round(float(min_similarity) * MILLION)) * count
        return {name: (int(group[i]) if keep[i] else None) for i, name in enumerate(self.queries)}

    def grown_own(self, stored):
        """``stored`` -- the ``GroupAffinity`` of the collection WITHOUT the queries, over the same groups -- grown by the gain: the own
        entries of the whole collection, ``stored own (+) gain`` for an old genome (sums added, the smaller lo, the larger hi) and this
        placement's own entry for a query, as a :class:`GrownOwn` over ``nodes``.  ValueError without the gain, for another direction,
        and for a stored partition that differs from this one on the old genomes."""
        if self.gain is None:
            raise ValueError("GroupPlacement.grown_own: the gain was not kept (want_gain)")
        if not isinstance(stored, GroupAffinity) or stored.is_distance != self.is_distance:
            raise ValueError("GroupPlacement.grown_own: stored must be a GroupAffinity of this placement's direction")
        is_query = np.zeros(len(self.nodes), dtype=bool)
        is_query[self.query_at] = True
        old = [name for name, q in zip(self.nodes, is_query) if not q]
        if sorted(stored.nodes) != sorted(old):
            raise ValueError("GroupPlacement.grown_own: the stored nodes are not this placement's old genomes")
        if len(stored.groups) != len(self.groups):
            raise ValueError(f"GroupPlacement.grown_own: the stored partition has {len(stored.groups)} groups, this one {len(self.groups)}")
        for name in stored.nodes:
            if int(stored.label[stored._at[name]]) != int(self.label[self._at[name]]):
                raise ValueError(f"GroupPlacement.grown_own: '{name}' is in group {int(stored.label[stored._at[name]])} of the stored partition and in "
                                 f"group {int(self.label[self._at[name]])} here")
        own_sum, own_lo, own_hi = (arr.astype(np.int64) for arr in self.gain)
        at = np.array([self._at[name] for name in stored.nodes], dtype=np.int64)
        own_sum[at] += stored.own_sum
        own_lo[at] = np.minimum(own_lo[at], stored.own_lo)
        own_hi[at] = np.maximum(own_hi[at], stored.own_hi)
        own_sum[self.query_at], own_lo[self.query_at], own_hi[self.query_at] = self.own_sum, self.own_lo, self.own_hi
        return GrownOwn(self.nodes, self.groups, own_sum, own_lo, own_hi, self.is_distance)


_PLACEMENT_COLUMNS = ["genome", "group", "position", "query", "own_sum", "own_min", "own_max", "mean_group", "mean_sum", "nearest_group", "nearest_value",
                      "farthest_group", "farthest_value", "gain_sum", "gain_min", "gain_max"]


def placement_to_file(placement, filepath):
    """The long form of a :class:`GroupPlacement` without its table: a first line ``#placement<TAB>G<TAB>distance|similarity<TAB>gain|nogain``,
    a header, then one line per node in node order -- its group's index and position in the group's given order (-1, -1: in no group),
    whether it is a query, a query's nine integers (``-`` for another node) and the node's gain (``-`` without it).
    ``placement_from_file`` gives the object back exactly."""
    where = {name: (b, k) for b, group in enumerate(placement.groups) for k, name in enumerate(group)}
    row_of = {name: k for k, name in enumerate(placement.queries)}
    with open(filepath, "w") as handle:
        handle.write(f"#placement\t{len(placement.groups)}\t{'distance' if placement.is_distance else 'similarity'}\t"
                     f"{'gain' if placement.gain is not None else 'nogain'}\n")
        handle.write("\t".join(_PLACEMENT_COLUMNS) + "\n")
        for i, name in enumerate(placement.nodes):
            b, position = where.get(name, (-1, -1))
            k = row_of.get(name)
            if k is None:
                mine = ["-"] * 9
            else:
                mine = [int(placement.own_sum[k]), int(placement.own_lo[k]), int(placement.own_hi[k]), int(placement.near_group[0, k]),
                        int(placement.near_sum[k]), int(placement.near_group[1, k]), int(placement.near_lo[k]), int(placement.near_group[2, k]),
                        int(placement.near_hi[k])]
            gain = ["-"] * 3 if placement.gain is None else [int(arr[i]) for arr in placement.gain]
            handle.write("\t".join(str(x) for x in (name, b, position, int(k is not None), *mine, *gain)) + "\n")
    return filepath


def placement_from_file(filepath):
    """The :class:`GroupPlacement` (without a table) of a file ``placement_to_file`` wrote.  ValueError for a file that is none."""
    with open(filepath, "r") as handle:
        first = next(handle, "").rstrip("\n").split("\t")
        if (len(first) != 4 or first[0] != "#placement" or first[2] not in ("distance", "similarity") or first[3] not in ("gain", "nogain") or
                not first[1].isdigit()):
            raise ValueError(f"{filepath}: no placement file (first line {first})")
        if next(handle, "").rstrip("\n").split("\t") != _PLACEMENT_COLUMNS:
            raise ValueError(f"{filepath}: no placement file (header)")
        rows = []
        for number, line in enumerate(handle, start=3):
            fields = line.rstrip("\n").split("\t")
            if len(fields) != len(_PLACEMENT_COLUMNS):
                raise ValueError(f"{filepath}:{number}: expected {len(_PLACEMENT_COLUMNS)} columns")
            rows.append(fields)
    g, has_gain = int(first[1]), first[3] == "gain"
    placed = [dict() for _ in range(g)]
    nodes, queries, mine, gain = [], [], [], []
    try:
        for fields in rows:
            name, b, position, is_query = fields[0], int(fields[1]), int(fields[2]), int(fields[3])
            nodes.append(name)
            if b != -1 or position != -1:
                if not 0 <= b < g or position in placed[b]:
                    raise ValueError(f"{filepath}: genome '{name}' at position {position} of group {b} of {g}")
                placed[b][position] = name
            if is_query:
                queries.append(name)
                mine.append([int(x) for x in fields[4:13]])
            if has_gain:
                gain.append([int(x) for x in fields[13:16]])
    except ValueError as exc:
        raise ValueError(f"{filepath}: no placement file ({exc})") from None
    if any(sorted(group) != list(range(len(group))) for group in placed):
        raise ValueError(f"{filepath}: a group's positions are not 0 .. size - 1")
    groups = [[group[k] for k in range(len(group))] for group in placed]
    cols = list(zip(*mine)) if mine else [()] * 9
    gain_cols = tuple(np.array(col, dtype=np.int64) for col in zip(*gain)) if has_gain and gain else ((np.empty(0, dtype=np.int64),) * 3 if has_gain else None)
    return GroupPlacement(nodes, groups, queries, cols[0], cols[1], cols[2], np.array([cols[3], cols[5], cols[7]], dtype=np.int32).reshape(3, len(queries)),
                          cols[4], cols[6], cols[8], gain=gain_cols, is_distance=first[2] == "distance")


def placement_de_novo(genomes, func, groups, queries=None, as_distance=True, want_table=False, want_gain=False, slab_bytes=0):
    """``GroupPlacement.from_dense(matrix_de_novo(genomes, func, cpus), groups, queries)`` -- with ``as_distance=False`` its ``inverted()``
    -- filling only the queries' rows: ``len(queries) * N`` pairs through ``Context.fill_rows_affinity``, neither the dense matrix nor
    the pairs among the other genomes.  ``groups``: each a sequence of genome names or of indices into ``genomes``, a genome in at most
    one; a genome in none is unlabelled.  ``queries`` (names or indices; default: the genomes in no group) are placed: a query may be
    labelled, and is then held against its own group's other members as ``affinity_de_novo`` holds it.  ``func`` must be one of the six
    ``METRICS`` callables.  One GPU: with several named the first; under a launcher (``WORLD_SIZE`` > 1) it raises.  Every refusal
    comes before the first GPU call."""
    names = [g.name for g in genomes]
    index = _name_index(names)
    members = _group_indices(names, index, groups)
    if len(members) < 1 or len(members) > BETWEEN_MAX_GROUPS:
        raise ValueError(f"placement_de_novo: {len(members)} groups (1..{BETWEEN_MAX_GROUPS})")
    label = np.full(len(names), -1, dtype=np.int32)
    for a, idx in enumerate(members):
        taken = [i for i in idx if label[i] >= 0]
        if taken:
            raise ValueError(f"placement_de_novo: genome '{names[taken[0]]}' is in groups {int(label[taken[0]])} and {a}")
        label[idx] = a
    if queries is None:
        rows = [int(i) for i in np.flatnonzero(label < 0)]
    else:
        (rows,) = _group_indices(names, index, [list(queries)])
    given = [[names[m] if isinstance(m, (int, np.integer)) else m for m in group] for group in groups]

    def fill(ctx, metric):
        result = ctx.fill_rows_affinity(metric, label, rows, len(members), as_distance=as_distance, slab_bytes=slab_bytes, want_table=want_table,
                                        want_gain=want_gain, want_stats=True)
        return result, result.pop("stats")

    _, (found,) = _de_novo_route(genomes, func, "placement_de_novo", fill,
        lambda stats, record, fill_s: f"{len(rows)} of {len(genomes)} genomes against {len(members)} groups -> {len(rows)} x {len(members)} entries on the "
                                      f"device from {stats['n_pairs']} of {record['genome_pairs']} pairs in {stats['n_slabs']} slab(s) on one device: "
                                      f"fill+passes+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, row passes "
                                      f"{stats.get('ms_rows', 0.0):.3f} ms, column passes {stats.get('ms_cols', 0.0):.3f} ms)",
        advice="for another callable: GroupPlacement.from_dense(matrix_de_novo(...), groups, queries)", several=False)
    return GroupPlacement(names, given, [names[i] for i in rows], found["own_sum"], found["own_lo"], found["own_hi"], found["near_group"], found["near_sum"],
                          found["near_lo"], found["near_hi"], table=found["table"], gain=found["gain"], is_distance=as_distance)


# ---- the command line's --place: a stored cluster fit as the partition, and the report of the new genomes ----
_FIT_COLUMNS = ["genome", "cluster", "own_similarity", "nearest_cluster", "nearest_similarity", "silhouette", "medoid"]
_REPORT_COLUMNS = ["genome", "mean_cluster", "mean_similarity", "nearest_cluster", "nearest_similarity", "farthest_cluster", "farthest_similarity",
                   "mean_cluster_size", "nearest_cluster_size", "farthest_cluster_size"]


def _value_text(value):
    return "nan" if value != value else repr(float(value))


def stored_fit_from_file(filepath):
    """What ``--place`` reads of a ``cluster_fit_<metric>.tsv``: ``(cluster names, groups, own)`` -- the clusters in the file's order, each
    group its genomes' names in the file's order, and ``own[name]`` the genome's own_similarity column as TEXT.  ValueError for a file
    that is none, and for a genome listed twice."""
    clusters, groups, own = [], [], {}
    with open(filepath, "r") as handle:
        if next(handle, "").rstrip("\n").split("\t") != _FIT_COLUMNS:
            raise ValueError(f"{filepath}: no cluster_fit file (header)")
        at = {}
        for number, line in enumerate(handle, start=2):
            fields = line.rstrip("\n").split("\t")
            if len(fields) != len(_FIT_COLUMNS):
                raise ValueError(f"{filepath}:{number}: expected {len(_FIT_COLUMNS)} columns")
            name, cluster = fields[0], fields[1]
            if name in own:
                raise ValueError(f"{filepath}:{number}: genome '{name}' is listed twice")
            if cluster not in at:
                at[cluster] = len(clusters)
                clusters.append(cluster)
                groups.append([])
            groups[at[cluster]].append(name)
            own[name] = fields[2]
    return clusters, groups, own


def own_similarity_text(placement, name):
    """A query's mean SIMILARITY to the other members of its own group, as ``--cluster-fit`` writes it (``GroupAffinity.own_mean`` of the
    similarity statement, ``repr``; ``nan`` for a genome alone in its group or in none)."""
    similar = placement if not placement.is_distance else placement.inverted()
    k = similar.queries.index(name)
    count = int(similar._own_count()[k])
    return _value_text(int(similar.own_sum[k]) / (count * MILLION) if count else float("nan"))


def placement_report(placement, cluster_names, genomes=None):
    """The lines of ``placement_<metric>.tsv``, header first: per query of ``genomes`` (default: every query), in their order, the nearest
    cluster by mean, by nearest and by farthest member, the three SIMILARITIES (from the integers: ``repr`` of the similarity
    statement's ``nearest_value``) and the three clusters' sizes; ``none`` / ``nan`` / 0 where there is no cluster."""
    similar = placement if not placement.is_distance else placement.inverted()
    groups = [similar.nearest_group(kind) for kind in AFFINITY_KINDS]
    values = [similar.nearest_value(kind) for kind in AFFINITY_KINDS]
    row_of = {name: k for k, name in enumerate(similar.queries)}
    lines = ["\t".join(_REPORT_COLUMNS)]
    for name in (similar.queries if genomes is None else genomes):
        k = row_of[name]
        cells = [name]
        for group, value in zip(groups, values):
            cells += [cluster_names[group[k]] if group[k] >= 0 else "none", _value_text(value[k])]
        cells += [str(int(similar.sizes[group[k]])) if group[k] >= 0 else "0" for group in groups]
        lines.append("\t".join(cells))
    return lines
