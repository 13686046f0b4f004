"""The affinity: how every genome relates to every group of a partition -- sum, minimum and maximum to its own group and the
nearest other group by three criteria -- without the dense matrix.

Owns ``GroupAffinity``, its route ``affinity_de_novo`` and its file (``affinity_to_file`` / ``affinity_from_file``)."""

import numpy as np

from phamclust_amd.routes import _de_novo_route, _partition_labels
from phamclust_amd.results.linkage import BETWEEN_MAX_GROUPS, MILLION, _EMPTY_HI, _EMPTY_LO, GroupLinkage

AFFINITY_KINDS = ("mean", "nearest", "farthest")       # the three criteria of a nearest group, in the order of ``near_group``'s rows


def _node_labels(nodes, at, groups):
    """int32 ``label[g]`` = the group of node g, ``at`` mapping a name to its position in ``nodes``: KeyError for a member that is no
    node, ValueError for a node in two groups or in none."""
    label = np.full(len(nodes), -1, dtype=np.int32)
    for b, group in enumerate(groups):
        for name in group:
            if name not in at:
                raise KeyError(f"GroupAffinity: '{name}' of group {b} is no node")
            if label[at[name]] >= 0:
                raise ValueError(f"GroupAffinity: '{name}' is in two groups")
            label[at[name]] = b
    if (label < 0).any():
        raise ValueError(f"GroupAffinity: '{nodes[int(np.flatnonzero(label < 0)[0])]}' is in no group")
    return label


class GroupAffinity:
    """How every genome of a collection relates to every group of a partition of it, in MILLIONTHS: what ``Context.fill_affinity``
    delivers and ``from_dense`` states on the host.  ``nodes`` are the genomes in array order, ``groups`` lists of their names (every
    node in exactly one group; a group may be empty); ``sizes[b]`` is a group's size and ``label[g]`` a genome's group.  Per genome:
    ``own_sum`` (int64), ``own_lo``, ``own_hi`` (int32) -- sum, minimum and maximum of its values to the other members of its own group
    -- and ``near_group`` (int32 ``[3, N]``): the OTHER non-empty group nearest by mean, by minimum and by maximum DISTANCE (ties to
    the smaller index, -1: none), with ``near_sum``, ``near_lo``, ``near_hi``, the value that made it nearest.  ``table``: None or the
    whole ``(sum, lo, hi)`` of ``[N, G]`` arrays; entry ``[g, b]`` counts ``sizes[b] - (label[g] == b)`` pairs, and one that counts none
    reads ``0, 2**31 - 1, -1``.  On similarities (``is_distance=False``) the groups are those of the inverted matrix and every value is
    the complement (``inverted``)."""

    def __init__(self, nodes, groups, own_sum, own_lo, own_hi, near_group, near_sum, near_lo, near_hi, table=None, is_distance=True):
        self.nodes = list(nodes)
        self.groups = [list(group) for group in groups]
        n, g = len(self.nodes), len(self.groups)
        at = {name: k for k, name in enumerate(self.nodes)}
        if len(at) != n:
            raise ValueError("GroupAffinity: node names must be distinct")
        self.label = _node_labels(self.nodes, at, self.groups)
        self._at = at
        self.sizes = np.array([len(group) for group in self.groups], dtype=np.int64)
        self.own_sum = np.ascontiguousarray(own_sum, dtype=np.int64)
        self.own_lo = np.ascontiguousarray(own_lo, dtype=np.int32)
        self.own_hi = np.ascontiguousarray(own_hi, dtype=np.int32)
        self.near_group = np.ascontiguousarray(near_group, dtype=np.int32)
        self.near_sum = np.ascontiguousarray(near_sum, dtype=np.int64)
        self.near_lo = np.ascontiguousarray(near_lo, dtype=np.int32)
        self.near_hi = np.ascontiguousarray(near_hi, dtype=np.int32)
        for name in ("own_sum", "own_lo", "own_hi", "near_sum", "near_lo", "near_hi"):
            if getattr(self, name).shape != (n,):
                raise ValueError(f"GroupAffinity: {name} must hold {n} entries, not {getattr(self, name).shape}")
        if self.near_group.shape != (3, n):
            raise ValueError(f"GroupAffinity: near_group must be 3 x {n}, not {self.near_group.shape}")
        self.table = None
        if table is not None:
            total, lo, hi = table
            self.table = (np.ascontiguousarray(total, dtype=np.int64), np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32))
            if any(arr.shape != (n, g) for arr in self.table):
                raise ValueError(f"GroupAffinity: the table must be three {n} x {g} arrays")
        self.is_distance = bool(is_distance)

    def __len__(self):
        return len(self.nodes)

    def _arrays(self):
        return (self.own_sum, self.own_lo, self.own_hi, self.near_group, self.near_sum, self.near_lo, self.near_hi)

    def __eq__(self, other):
        return (isinstance(other, GroupAffinity) and self.nodes == other.nodes and self.groups == other.groups and self.is_distance == other.is_distance and
                all(np.array_equal(a, b) for a, b in zip(self._arrays(), other._arrays())) and (self.table is None) == (other.table is None) and
                (self.table is None or all(np.array_equal(a, b) for a, b in zip(self.table, other.table))))

    __hash__ = None

    def counts(self):
        """``[N, G]``: the pairs entry ``[g, b]`` counts, ``sizes[b] - (label[g] == b)``."""
        count = np.broadcast_to(self.sizes, (len(self.nodes), len(self.groups))).copy()
        count[np.arange(len(self.nodes)), self.label] -= 1
        return count

    def _own_count(self):
        return self.sizes[self.label] - 1

    @classmethod
    def _from_distance_table(cls, nodes, groups, total, lo, hi, is_distance, keep_table):
        """The O(N) statement read off the DISTANCE table (int64 ``[N, G]``, empty entries in the empty convention); a similarity
        result is its ``inverted()``."""
        g = len(groups)
        n = len(nodes)
        label = _node_labels(nodes, {name: k for k, name in enumerate(nodes)}, groups)
        sizes = np.array([len(group) for group in groups], dtype=np.int64)
        rows = np.arange(n)
        best = [np.full(n, -1, dtype=np.int64) for _ in range(3)]
        b_sum, b_size = np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)
        b_lo, b_hi = np.full(n, _EMPTY_LO, dtype=np.int64), np.full(n, _EMPTY_LO, dtype=np.int64)
        for b in range(g):                                                  # ascending, strictly better only: ties stay with the smaller index
            if not sizes[b]:
                continue
            other = label != b
            take = other & ((best[0] < 0) | (total[:, b] * b_size < b_sum * sizes[b]))      # sum_b / size_b < sum_c / size_c, in integers
            best[0][take], b_sum[take], b_size[take] = b, total[take, b], sizes[b]
            take = other & ((best[1] < 0) | (lo[:, b] < b_lo))
            best[1][take], b_lo[take] = b, lo[take, b]
            take = other & ((best[2] < 0) | (hi[:, b] < b_hi))
            best[2][take], b_hi[take] = b, hi[take, b]
        none = best[0] < 0
        out = cls(nodes, groups, total[rows, label], lo[rows, label], hi[rows, label], np.stack(best), np.where(none, 0, b_sum),
                  np.where(none, _EMPTY_LO, b_lo), np.where(none, _EMPTY_HI, b_hi), table=(total, lo, hi) if keep_table else None, is_distance=True)
        return out if is_distance else out.inverted()

    @classmethod
    def from_dense(cls, matrix, groups, want_table=True):
        """The host statement of the definition, in integers, by numpy: the affinity of ``groups`` (lists of names of ``matrix``, every
        node in exactly one) over the weights of ``matrix``, the nodes in the matrix's order.  A similarity matrix gives the statement
        of its ``invert()``, inverted.  ValueError for a weight that is unset or no millionth."""
        groups = [list(group) for group in groups]
        nodes = matrix.nodes
        data = np.asarray(matrix._ordered(), dtype=np.float64)
        n = len(nodes)
        micro = np.rint(data * 1.0e6)
        exact = micro / 1.0e6 == data
        np.fill_diagonal(exact, True)                                       # the diagonal: no pair
        np.fill_diagonal(micro, 0.0)
        if not (micro >= 0.0).all() or not (micro <= 1.0e6).all() or not exact.all():
            raise ValueError("GroupAffinity.from_dense: a weight is unset or no millionth in [0, 1]")
        del exact
        micro = micro.astype(np.int64)
        if not matrix.is_distance:
            micro = MILLION - micro
        at = {name: k for k, name in enumerate(nodes)}
        for group in groups:
            for name in group:
                if name not in at:
                    raise KeyError(f"node '{name}' not in matrix")
        g = len(groups)
        order = np.array([at[name] for group in groups for name in group], dtype=np.int64)
        if order.shape[0] != n or np.unique(order).shape[0] != n:
            raise ValueError("GroupAffinity.from_dense: every node must be in exactly one group")
        sizes = np.array([len(group) for group in groups], dtype=np.int64)
        present = np.flatnonzero(sizes > 0)
        starts = (np.cumsum(sizes) - sizes)[present]
        micro = micro[:, order]                                             # the columns group by group
        own = (order, np.arange(n))                                         # where a genome meets itself: no pair
        total = np.zeros((n, g), dtype=np.int64)
        lo = np.full((n, g), _EMPTY_LO, dtype=np.int64)
        hi = np.full((n, g), _EMPTY_HI, dtype=np.int64)
        if n:
            micro[own] = 0
            total[:, present] = np.add.reduceat(micro, starts, axis=1)
            micro[own] = _EMPTY_LO
            lo[:, present] = np.minimum.reduceat(micro, starts, axis=1)
            micro[own] = _EMPTY_HI
            hi[:, present] = np.maximum.reduceat(micro, starts, axis=1)
        del micro
        return cls._from_distance_table(nodes, groups, total, lo, hi, matrix.is_distance, want_table)

    def inverted(self):
        """distance <-> similarity: the same nearest groups, every value complemented -- ``sum' = count * 10^6 - sum``; the own entries
        and the table ``lo' = 10^6 - hi``, ``hi' = 10^6 - lo``; ``near_lo' = 10^6 - near_lo`` and ``near_hi' = 10^6 - near_hi`` (each is
        the value of ITS group); empty entries stay empty."""
        def flipped(total, lo, hi, count):
            full = count > 0
            return (np.where(full, count * MILLION - total, 0), np.where(full, MILLION - hi.astype(np.int64), _EMPTY_LO),
                    np.where(full, MILLION - lo.astype(np.int64), _EMPTY_HI))
        own = flipped(self.own_sum, self.own_lo, self.own_hi, self._own_count())
        near = self.near_group[0] >= 0
        near_size = np.where(near, self.sizes[np.maximum(self.near_group[0], 0)] if len(self.sizes) else 0, 0)
        table = None if self.table is None else flipped(*self.table, self.counts())
        return GroupAffinity(self.nodes, self.groups, *own, self.near_group, np.where(near, near_size * MILLION - self.near_sum, 0),
                             np.where(near, MILLION - self.near_lo.astype(np.int64), _EMPTY_LO), np.where(near, MILLION - self.near_hi.astype(np.int64), _EMPTY_HI),
                             table=table, is_distance=not self.is_distance)

    def medoids(self):
        """Per group its medoid's name (None for an empty group): the member with the smallest own sum on distances, the largest on
        similarities -- ``SymMatrix.medoid`` of the group's sub-matrix; a tie goes to the first member in the group's given order, and
        a one-member group is its own medoid."""
        out = []
        for group in self.groups:
            if not group:
                out.append(None)
                continue
            sums = self.own_sum[[self._at[name] for name in group]]
            out.append(group[int(np.argmin(sums) if self.is_distance else np.argmax(sums))])
        return out

    def own_mean(self, name):
        """A genome's mean value to the other members of its own group; ``nan`` for a genome alone in its group."""
        k = self._at[name]
        count = int(self._own_count()[k])
        return int(self.own_sum[k]) / (count * MILLION) if count else float("nan")

    @staticmethod
    def _kind(kind, who):
        if kind not in AFFINITY_KINDS:
            raise ValueError(f"GroupAffinity.{who}: kind must be 'mean', 'nearest' or 'farthest', not {kind!r}")
        return AFFINITY_KINDS.index(kind)

    def nearest_group(self, kind="mean"):
        """``[N]`` int32: the other non-empty group nearest by ``kind`` -- ``'mean'`` (average linkage), ``'nearest'`` (single) or
        ``'farthest'`` (complete linkage to the group); -1 where there is none."""
        return self.near_group[self._kind(kind, "nearest_group")].copy()

    def nearest_value(self, kind="mean"):
        """``[N]`` float64: the value that made ``nearest_group(kind)`` nearest -- the mean value to it, the best single value, or the
        worst; ``nan`` where there is no other group."""
        k = self._kind(kind, "nearest_value")
        group = self.near_group[k]
        there = group >= 0
        out = np.full(len(self.nodes), np.nan)
        if k == 0:
            out[there] = self.near_sum[there] / (self.sizes[group[there]] * float(MILLION))
        else:
            out[there] = (self.near_lo if k == 1 else self.near_hi)[there] / float(MILLION)
        return out

    def silhouette(self):
        """``[N]`` float64: ``(b - a) / max(a, b)`` per genome, with a its mean DISTANCE to its own group and b the smallest mean distance
        to another, from the integers; 0 for a genome alone in its group (scikit-learn's convention) and where ``max(a, b) == 0``;
        ``nan`` everywhere when fewer than two groups are non-empty."""
        n = len(self.nodes)
        if int((self.sizes > 0).sum()) < 2:
            return np.full(n, np.nan)
        dist = self if self.is_distance else self.inverted()
        count = dist._own_count()
        a = dist.own_sum / (np.maximum(count, 1) * float(MILLION))
        b = dist.near_sum / (dist.sizes[dist.near_group[0]] * float(MILLION))
        top = np.maximum(a, b)
        out = np.zeros(n)
        ok = (count > 0) & (top > 0.0)
        out[ok] = (b[ok] - a[ok]) / top[ok]
        return out

    def silhouette_by_group(self):
        """Per group the mean silhouette of its members (``nan`` for an empty group)."""
        s = self.silhouette()
        return [float(np.mean(s[[self._at[name] for name in group]])) if group else float("nan") for group in self.groups]

    def silhouette_mean(self):
        """The mean silhouette over all genomes."""
        s = self.silhouette()
        return float(np.mean(s)) if s.size else float("nan")

    def folded(self):
        """The :class:`GroupLinkage` of the same partition, from the table: the rows of a group summed (extremes combined) give the
        between table's row, off-diagonal entries as they are, the diagonal -- every pair met from both ends -- halved."""
        if self.table is None:
            raise ValueError("GroupAffinity.folded: the table was not kept (want_table)")
        total, lo, hi = self.table
        g = len(self.groups)
        out_sum = np.zeros((g, g), dtype=np.int64)
        out_lo = np.full((g, g), _EMPTY_LO, dtype=np.int32)
        out_hi = np.full((g, g), _EMPTY_HI, dtype=np.int32)
        for a, group in enumerate(self.groups):
            if group:
                rows = [self._at[name] for name in group]
                out_sum[a], out_lo[a], out_hi[a] = total[rows].sum(axis=0), lo[rows].min(axis=0), hi[rows].max(axis=0)
        count = np.outer(self.sizes, self.sizes)
        np.fill_diagonal(count, self.sizes * (self.sizes - 1) // 2)
        np.fill_diagonal(out_sum, np.diagonal(out_sum) // 2)
        return GroupLinkage(self.groups, out_sum, count, out_lo, out_hi, is_distance=self.is_distance)


_AFFINITY_COLUMNS = ["genome", "group", "position", "own_sum", "own_min", "own_max", "mean_group", "mean_sum", "nearest_group", "nearest_value",
                     "farthest_group", "farthest_value"]


def affinity_to_file(affinity, filepath):
    """The long form of a :class:`GroupAffinity`'s O(N) arrays (not its table): a first line ``#affinity<TAB>G<TAB>distance|similarity``,
    a header, then one line per genome in node order -- its group's index and its position in the group's given order, then the seven
    integers and three group indices as they are.  ``affinity_from_file`` gives the object back exactly."""
    where = {name: (b, k) for b, group in enumerate(affinity.groups) for k, name in enumerate(group)}
    with open(filepath, "w") as handle:
        handle.write(f"#affinity\t{len(affinity.groups)}\t{'distance' if affinity.is_distance else 'similarity'}\n")
        handle.write("\t".join(_AFFINITY_COLUMNS) + "\n")
        for k, name in enumerate(affinity.nodes):
            b, position = where[name]
            handle.write(f"{name}\t{b}\t{position}\t{int(affinity.own_sum[k])}\t{int(affinity.own_lo[k])}\t{int(affinity.own_hi[k])}\t"
                         f"{int(affinity.near_group[0, k])}\t{int(affinity.near_sum[k])}\t{int(affinity.near_group[1, k])}\t{int(affinity.near_lo[k])}\t"
                         f"{int(affinity.near_group[2, k])}\t{int(affinity.near_hi[k])}\n")
    return filepath


def affinity_from_file(filepath):
    """The :class:`GroupAffinity` (without a table) of a file ``affinity_to_file`` wrote.  ValueError for a file that is none."""
    with open(filepath, "r") as handle:
        first = next(handle, "").rstrip("\n").split("\t")
        if len(first) != 3 or first[0] != "#affinity" or first[2] not in ("distance", "similarity") or not first[1].isdigit():
            raise ValueError(f"{filepath}: no affinity file (first line {first})")
        if next(handle, "").rstrip("\n").split("\t") != _AFFINITY_COLUMNS:
            raise ValueError(f"{filepath}: no affinity file (header)")
        rows = []
        for number, line in enumerate(handle, start=3):
            fields = line.rstrip("\n").split("\t")
            if len(fields) != len(_AFFINITY_COLUMNS):
                raise ValueError(f"{filepath}:{number}: expected {len(_AFFINITY_COLUMNS)} columns")
            rows.append((fields[0], *(int(x) for x in fields[1:])))
    g = int(first[1])
    placed = [dict() for _ in range(g)]
    for name, b, position, *_ in rows:
        if not 0 <= b < g or position in placed[b]:
            raise ValueError(f"{filepath}: genome '{name}' at position {position} of group {b} of {g}")
        placed[b][position] = name
    if any(sorted(group) != list(range(len(group))) for group in placed):
        raise ValueError(f"{filepath}: a group's positions are not 0 .. size - 1")
    groups = [[group[k] for k in range(len(group))] for group in placed]
    cols = list(zip(*[row[3:] for row in rows])) if rows else [()] * 9
    return GroupAffinity([row[0] for row in rows], groups, cols[0], cols[1], cols[2], np.array([cols[3], cols[5], cols[7]], dtype=np.int32).reshape(3, len(rows)),
                         cols[4], cols[6], cols[8], is_distance=first[2] == "distance")


def affinity_de_novo(genomes, func, groups, as_distance=True, slab_bytes=0, want_table=False):
    """``GroupAffinity.from_dense(matrix_de_novo(genomes, func, cpus), groups)`` -- with ``as_distance=False`` its ``inverted()`` -- without
    the dense matrix: ``groups`` is a partition of the genomes, each group a sequence of genome names or of indices into ``genomes``,
    every genome in exactly one group, filled on the GPU by ``Context.fill_affinity``.  The N x G table stays on the device; the O(N)
    arrays cross PCIe, and with ``want_table`` the table too.  ``func`` must be one of the six ``METRICS`` callables.  Several devices as
    ``between_de_novo`` (``MultiContext.fill_affinity``: the same result); under a launcher (``WORLD_SIZE`` > 1) it raises.  Every
    refusal comes before the first GPU call."""
    names = [g.name for g in genomes]
    members, label = _partition_labels(names, groups, "affinity_de_novo", BETWEEN_MAX_GROUPS)

    def fill(ctx, metric):
        result = ctx.fill_affinity(metric, label, len(members), as_distance=as_distance, slab_bytes=slab_bytes, want_table=want_table, want_stats=True)
        return result, result.pop("stats")

    _, (found,) = _de_novo_route(genomes, func, "affinity_de_novo", fill,
        lambda stats, record, fill_s: f"{len(genomes)} genomes in {len(members)} groups -> {len(genomes)} x {len(members)} entries on the device from "
                                      f"{record['genome_pairs']} pairs in {stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): "
                                      f"fill+passes+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, row passes "
                                      f"{stats.get('ms_rows', 0.0):.3f} ms, column passes {stats.get('ms_cols', 0.0):.3f} ms)",
        advice="for another callable: GroupAffinity.from_dense(matrix_de_novo(...), groups)")
    given = [[names[m] if isinstance(m, (int, np.integer)) else m for m in group] for group in groups]      # (the given order decides a medoid's tie)
    return GroupAffinity(names, given, found["own_sum"], found["own_lo"], found["own_hi"], found["near_group"], found["near_sum"], found["near_lo"],
                         found["near_hi"], table=found["table"], is_distance=as_distance)
