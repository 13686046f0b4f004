"""The table between the groups of a partition: count, sum, minimum and maximum of the pair values of every two groups.

Owns ``GroupLinkage``, its routes ``between_de_novo`` and ``between_extend`` (a stored table grown by new genomes) and its file (``between_to_file`` / ``between_from_file``); ``MILLION`` and
the empty entry's ``_EMPTY_LO`` / ``_EMPTY_HI`` are shared with the affinity result."""

import logging

import numpy as np

from phamclust_amd.symmatrix import _square_matrix
from phamclust_amd.routes import LAST_FILL, _de_novo_route, _partition_labels

BETWEEN_MAX_GROUPS = 2048   # PC_BETWEEN_MAX_GROUPS of the C-ABI: the groups a between-groups fill takes at most
MILLION = 1000000
_EMPTY_LO, _EMPTY_HI = 2 ** 31 - 1, -1


class GroupLinkage:
    """For a partition of a collection into ``groups`` (lists of names) the ``[G, G]`` table of the pair values between every two
    groups, and within each group on the diagonal, in MILLIONTHS: ``sum`` and ``count`` (int64), ``lo`` and ``hi`` (int32), symmetric --
    what ``Context.fill_between`` delivers and ``from_dense`` states on the host.  Every weight of a matrix is ``round(x, 6)``, so the
    table is exact integers.  ``lo`` is the single-linkage, ``hi`` the complete-linkage and ``sum / count`` the average-linkage value
    of two groups.  An entry no pair fell into (the diagonal of a one-member group, any entry of an empty group) reads ``count = 0,
    sum = 0, lo = 2**31 - 1, hi = -1``."""

    def __init__(self, groups, sum, count, lo, hi, is_distance=True):
        self.groups = [list(group) for group in groups]
        g = len(self.groups)
        self.sum = np.ascontiguousarray(sum, dtype=np.int64)
        self.cnt = np.ascontiguousarray(count, dtype=np.int64)
        self.lo = np.ascontiguousarray(lo, dtype=np.int32)
        self.hi = np.ascontiguousarray(hi, dtype=np.int32)
        self.is_distance = bool(is_distance)
        for name, arr in (("sum", self.sum), ("count", self.cnt), ("lo", self.lo), ("hi", self.hi)):
            if arr.shape != (g, g):
                raise ValueError(f"GroupLinkage: {name} must be {g} x {g} for {g} groups, not {arr.shape}")
            if not np.array_equal(arr, arr.T):
                raise ValueError(f"GroupLinkage: {name} is not symmetric")

    def __len__(self):
        return len(self.groups)

    def __eq__(self, other):
        return (isinstance(other, GroupLinkage) and self.groups == other.groups and self.is_distance == other.is_distance and
                all(np.array_equal(a, b) for a, b in ((self.sum, other.sum), (self.cnt, other.cnt), (self.lo, other.lo), (self.hi, other.hi))))

    __hash__ = None

    def _full(self, a, b, what):
        if not self.cnt[a, b]:
            raise ValueError(f"GroupLinkage.{what}: no pair lies between groups {a} and {b}")

    def count(self, a, b):
        """Pairs between groups ``a`` and ``b`` (``a == b``: within the group)."""
        return int(self.cnt[a, b])

    def mean(self, a, b):
        """Their mean value: ``sum / (count * 10^6)``, one division of exact integers."""
        self._full(a, b, "mean")
        return int(self.sum[a, b]) / (int(self.cnt[a, b]) * MILLION)

    def nearest(self, a, b):
        """The better extreme: the smallest distance, or the largest similarity (single linkage)."""
        self._full(a, b, "nearest")
        return int(self.lo[a, b] if self.is_distance else self.hi[a, b]) / MILLION

    def farthest(self, a, b):
        """The worse extreme: the largest distance, or the smallest similarity (complete linkage)."""
        self._full(a, b, "farthest")
        return int(self.hi[a, b] if self.is_distance else self.lo[a, b]) / MILLION

    def diameter(self, a):
        """``SymMatrix.diameter`` of the group's sub-matrix: its largest distance, 0.0 for fewer than two members."""
        if not self.is_distance:
            raise ValueError("cannot compute diameter for similarity matrix")
        return int(self.hi[a, a]) / MILLION if self.cnt[a, a] else 0.0

    def within_mean(self, a):
        """``SymMatrix.statistics[0]`` of the group's sub-matrix: the mean of its pairs; for a one-member group the diagonal's value."""
        return self.mean(a, a) if self.cnt[a, a] else 1.0 - self.is_distance

    def to_symmatrix(self, names, kind="mean"):
        """The table as a ``SymMatrix`` over the group ``names``: ``kind`` ``"mean"``, ``"nearest"`` or ``"farthest"`` of every two
        groups, six places as every weight; the diagonal is the within-group mean, ``1 - is_distance`` for a one-member group.  What
        ``draw_heatmap`` and ``matrix_to_squareform`` take.  An empty group has no values: ValueError."""
        names = list(names)
        g = len(self)
        if len(names) != g or len(set(names)) != g:
            raise ValueError(f"GroupLinkage.to_symmatrix: need {g} distinct names")
        value = {"mean": self.mean, "nearest": self.nearest, "farthest": self.farthest}.get(kind)
        if value is None:
            raise ValueError(f"GroupLinkage.to_symmatrix: kind must be 'mean', 'nearest' or 'farthest', not {kind!r}")
        data = np.empty((g, g), dtype=np.float64)
        for a in range(g):
            if not self.groups[a]:
                raise ValueError(f"GroupLinkage.to_symmatrix: group {a} ('{names[a]}') is empty")
            data[a, a] = round(self.within_mean(a), 6)
            for b in range(a + 1, g):
                data[a, b] = data[b, a] = round(value(a, b), 6) if self.cnt[a, b] else np.nan
        return _square_matrix(names, data, self.is_distance)

    def merged(self, parts):
        """The exact table of a coarser partition: ``parts`` are lists of group indices, each group in at most one part (a group in
        none is left out).  Sums and counts add, extremes combine; a merged group's diagonal takes in the entries between its parts."""
        parts = [[int(a) for a in part] for part in parts]
        flat = [a for part in parts for a in part]
        g = len(self)
        if any(not 0 <= a < g for a in flat) or len(set(flat)) != len(flat):
            raise ValueError("GroupLinkage.merged: parts must hold distinct group indices of this table")
        member = np.zeros((len(parts), g), dtype=np.int64)
        for p, part in enumerate(parts):
            member[p, part] = 1

        def added(table):
            square = member @ table @ member.T                 # (int64, exact) a diagonal entry: within its parts once, between them twice
            within = member @ np.diagonal(table)
            out = square.copy()
            np.fill_diagonal(out, (np.diagonal(square) + within) // 2)
            return out

        def extreme(table, reduce, empty):
            rows = np.stack([reduce(table[part, :], axis=0, initial=empty) if part else np.full(g, empty, dtype=table.dtype) for part in parts]) \
                if parts else np.empty((0, g), dtype=table.dtype)
            cols = [reduce(rows[:, part], axis=1, initial=empty) if part else np.full(len(parts), empty, dtype=table.dtype) for part in parts]
            return np.stack(cols, axis=1).astype(np.int32) if parts else np.empty((0, 0), dtype=np.int32)

        groups = [[name for a in part for name in self.groups[a]] for part in parts]
        return GroupLinkage(groups, added(self.sum), added(self.cnt), extreme(self.lo, np.min, _EMPTY_LO), extreme(self.hi, np.max, _EMPTY_HI),
                            is_distance=self.is_distance)

    def inverted(self):
        """distance <-> similarity: every weight w = k / 10^6 becomes (10^6 - k) / 10^6 (``round(1 - w, 6)``), so ``sum' = count * 10^6 -
        sum``, ``lo' = 10^6 - hi`` and ``hi' = 10^6 - lo``; empty entries stay empty."""
        full = self.cnt > 0
        lo = np.where(full, MILLION - self.hi.astype(np.int64), _EMPTY_LO).astype(np.int32)
        hi = np.where(full, MILLION - self.lo.astype(np.int64), _EMPTY_HI).astype(np.int32)
        return GroupLinkage(self.groups, self.cnt * MILLION - self.sum, self.cnt, lo, hi, is_distance=not self.is_distance)

    def padded(self, n_groups):
        """The four arrays with empty entries appended up to ``n_groups`` groups (at least this table's)."""
        g = len(self)
        if n_groups < g:
            raise ValueError(f"GroupLinkage.padded: {n_groups} groups are fewer than this table's {g}")
        out = []
        for arr, empty in ((self.sum, 0), (self.cnt, 0), (self.lo, _EMPTY_LO), (self.hi, _EMPTY_HI)):
            wide = np.full((n_groups, n_groups), empty, dtype=arr.dtype)
            wide[:g, :g] = arr
            out.append(wide)
        return tuple(out)

    def _grown_members(self, groups, who):
        """``groups`` as a grown partition of this table's: group i of the table a subset of group i, more groups may follow.  Returns the
        set of stored members.  ValueError for fewer groups, a genome in two groups, a stored member that is missing or moved."""
        groups = [list(group) for group in groups]
        if len(groups) < len(self):
            raise ValueError(f"{who}: {len(groups)} groups are fewer than the stored table's {len(self)}")
        where = {}
        for a, group in enumerate(groups):
            for name in group:
                if name in where:
                    raise ValueError(f"{who}: '{name}' is in groups {where[name]} and {a}")
                where[name] = a
        stored = set()
        for a, group in enumerate(self.groups):
            for name in group:
                if name not in where:
                    raise ValueError(f"{who}: stored member '{name}' of group {a} is missing from the grown partition (a stored table cannot "
                                     "lose a genome: a minimum cannot be un-taken)")
                if where[name] != a:
                    raise ValueError(f"{who}: stored member '{name}' of group {a} moved to group {where[name]}")
                if name in stored:
                    raise ValueError(f"{who}: stored member '{name}' is listed twice")
                stored.add(name)
        return stored

    def extended(self, matrix, groups):
        """This table grown to ``groups``, a partition of (some of) the nodes of ``matrix`` -- any dense ``SymMatrix`` over the grown
        collection, of this table's direction: group i of this table must be a subset of ``groups[i]``, and more groups may follow.  The
        new genomes are the members of ``groups`` this table does not hold; the result is the stored integers plus the NEW genomes' rows
        of ``matrix`` alone -- counts and sums add, extremes only move outward -- and equals ``GroupLinkage.from_dense(matrix, groups)``.
        ValueError for a stored member that is missing or moved, for another direction, and for a new genome's weight that is unset or
        no millionth."""
        groups = [list(group) for group in groups]
        if bool(matrix.is_distance) != self.is_distance:
            raise ValueError("GroupLinkage.extended: the matrix holds " + ("distances" if matrix.is_distance else "similarities") +
                             ", the stored table " + ("distances" if self.is_distance else "similarities"))
        stored = self._grown_members(groups, "GroupLinkage.extended")
        g, n = len(groups), matrix._data.shape[0]
        label = np.full(n, -1, dtype=np.int64)
        is_new = np.zeros(n, dtype=bool)
        for a, group in enumerate(groups):
            for name in group:
                if name not in matrix:
                    raise KeyError(f"node '{name}' not in matrix")
                label[matrix._slot[name]] = a
                is_new[matrix._slot[name]] = name not in stored
        total, count, lo, hi = (arr.astype(np.int64) for arr in self.padded(g))
        rows = np.flatnonzero(is_new)
        if rows.shape[0]:
            block = matrix._data[rows, :]
            cols = np.arange(n)
            # a new genome's row takes the pairs to every labelled genome but itself; a pair of two new genomes is the smaller slot's
            live = (label[None, :] >= 0) & (cols[None, :] != rows[:, None]) & ((cols[None, :] > rows[:, None]) | ~is_new[None, :])
            values = block[live]
            micro = np.rint(values * 1.0e6)
            if not (micro >= 0.0).all() or not (micro <= 1.0e6).all() or not np.array_equal(micro / 1.0e6, values):
                raise ValueError("GroupLinkage.extended: a weight of a new genome is unset or no millionth in [0, 1]")
            micro = micro.astype(np.int64)
            a = np.broadcast_to(label[rows][:, None], live.shape)[live]
            b = np.broadcast_to(label[None, :], live.shape)[live]
            first, second = np.minimum(a, b), np.maximum(a, b)
            flat = first * g + second
            add_count = np.bincount(flat, minlength=g * g).astype(np.int64)
            add_total = np.zeros(g * g, dtype=np.int64)
            np.add.at(add_total, flat, micro)
            add_lo = np.full(g * g, _EMPTY_LO, dtype=np.int64)
            add_hi = np.full(g * g, _EMPTY_HI, dtype=np.int64)
            np.minimum.at(add_lo, flat, micro)
            np.maximum.at(add_hi, flat, micro)
            upper = np.triu(np.ones((g, g), dtype=bool))

            def both(square):                                              # entries a <= b were written: mirror them
                square = square.reshape(g, g)
                return np.where(upper, square, square.T)
            count += both(add_count)
            total += both(add_total)
            lo = np.minimum(lo, both(add_lo))
            hi = np.maximum(hi, both(add_hi))
        return GroupLinkage(groups, total, count, lo.astype(np.int32), hi.astype(np.int32), is_distance=self.is_distance)

    @classmethod
    def from_dense(cls, matrix, groups):
        """The host statement of the definition, in numpy: the table of ``groups`` (lists of names of ``matrix``, each name in at most
        one group; a name in none takes no part) over the weights of ``matrix``.  ValueError for a weight that is unset or no millionth."""
        groups = [list(group) for group in groups]
        n = matrix._data.shape[0]
        label = np.full(n, -1, dtype=np.int64)
        for a, group in enumerate(groups):
            for name in group:
                if name not in matrix:
                    raise KeyError(f"node '{name}' not in matrix")
                if label[matrix._slot[name]] >= 0:
                    raise ValueError(f"GroupLinkage.from_dense: '{name}' is in two groups")
                label[matrix._slot[name]] = a
        g = len(groups)
        order = np.flatnonzero(label >= 0)
        order = order[np.argsort(label[order], kind="stable")]             # the members, group by group
        sizes = np.bincount(label[order], minlength=g) if g else np.zeros(0, dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)])[:-1] if g else np.zeros(0, dtype=np.int64)
        present = np.flatnonzero(sizes > 0)
        total = np.zeros((g, g), dtype=np.int64)
        count = np.zeros((g, g), dtype=np.int64)
        lo = np.full((g, g), _EMPTY_LO, dtype=np.int64)
        hi = np.full((g, g), _EMPTY_HI, dtype=np.int64)
        at = np.empty(n, dtype=np.int64)
        at[order] = np.arange(order.shape[0])
        for a in present.tolist():
            rows = order[starts[a]:starts[a] + sizes[a]]
            block = matrix._data[np.ix_(rows, order)]                      # this group's members against all, columns group by group
            micro = np.rint(block * 1.0e6)
            own = (np.arange(rows.shape[0]), at[rows])                      # the diagonal: no pair
            check = block.copy()
            check[own] = 0.0
            micro[own] = 0.0
            if not (micro >= 0.0).all() or not (micro <= 1.0e6).all() or not np.array_equal(micro / 1.0e6, check):
                raise ValueError("GroupLinkage.from_dense: a weight is unset or no millionth in [0, 1]")
            micro = micro.astype(np.int64)
            total[a, present] = np.add.reduceat(micro.sum(axis=0), starts[present])
            count[a, present] = sizes[a] * sizes[present]
            small, large = micro.copy(), micro
            small[own] = _EMPTY_LO
            large[own] = _EMPTY_HI
            lo[a, present] = np.minimum.reduceat(small.min(axis=0), starts[present])
            hi[a, present] = np.maximum.reduceat(large.max(axis=0), starts[present])
            total[a, a] //= 2                                               # within the group every pair was met from both ends
            count[a, a] = sizes[a] * (sizes[a] - 1) // 2
            if sizes[a] == 1:
                lo[a, a], hi[a, a] = _EMPTY_LO, _EMPTY_HI
        return cls(groups, total, count, lo.astype(np.int32), hi.astype(np.int32), is_distance=matrix.is_distance)


def between_to_file(table, names, filepath):
    """``cluster_table_<metric>.tsv``, the long form of a :class:`GroupLinkage`: a header, then one line ``group_a<TAB>group_b<TAB>count
    <TAB>mean<TAB>min<TAB>max<TAB>sum`` per pair of groups a <= b in the order of ``names`` (the diagonal: within the group).  ``mean`` is
    written with all its digits (``repr``: nine significant digits do not tell two means apart), ``min`` and ``max`` with six places, and
    ``sum`` -- the integer sum of the values' millionths -- makes the file exact: ``between_from_file`` gives the table back bit for bit.
    An entry without pairs reads ``0  nan  nan  nan  0``."""
    names = list(names)
    if len(names) != len(table) or len(set(names)) != len(names):
        raise ValueError(f"between_to_file: need {len(table)} distinct names")
    with open(filepath, "w") as handle:
        handle.write("group_a\tgroup_b\tcount\tmean\tmin\tmax\tsum\n")
        for a, first in enumerate(names):
            for b in range(a, len(names)):
                if table.cnt[a, b]:
                    handle.write(f"{first}\t{names[b]}\t{int(table.cnt[a, b])}\t{table.mean(a, b)!r}\t{int(table.lo[a, b]) / MILLION:.6f}\t"
                                 f"{int(table.hi[a, b]) / MILLION:.6f}\t{int(table.sum[a, b])}\n")
                else:
                    handle.write(f"{first}\t{names[b]}\t0\tnan\tnan\tnan\t0\n")
    return filepath


def between_from_file(filepath, groups=None, is_distance=True):
    """``(names, GroupLinkage)`` of a file ``between_to_file`` wrote: the group names in file order and the table, bit for bit.  The file
    does not hold the members: ``groups`` (lists of names, in the file's group order) supplies them; without it every group holds its
    own name.  ``is_distance``: what the file's values are.  ValueError for a file that is no such table."""
    names, index, rows = [], {}, []
    with open(filepath, "r") as handle:
        header = next(handle, "").rstrip("\n").split("\t")
        if header != ["group_a", "group_b", "count", "mean", "min", "max", "sum"]:
            raise ValueError(f"{filepath}: no cluster table (header {header})")
        for number, line in enumerate(handle, start=2):
            fields = line.rstrip("\n").split("\t")
            if len(fields) != 7:
                raise ValueError(f"{filepath}:{number}: expected 7 columns")
            for name in fields[:2]:
                if name not in index:
                    index[name] = len(names)
                    names.append(name)
            count, total = int(fields[2]), int(fields[6])
            if count:
                low, high = int(np.rint(float(fields[4]) * 1.0e6)), int(np.rint(float(fields[5]) * 1.0e6))
            else:
                low, high = _EMPTY_LO, _EMPTY_HI
            rows.append((index[fields[0]], index[fields[1]], count, total, low, high))
    g = len(names)
    if len(rows) != g * (g + 1) // 2 or len({(a, b) for a, b, *_ in rows}) != len(rows) or any(a > b for a, b, *_ in rows):
        raise ValueError(f"{filepath}: {len(rows)} lines are not the pairs a <= b of {g} groups")
    total = np.zeros((g, g), dtype=np.int64)
    count = np.zeros((g, g), dtype=np.int64)
    lo = np.full((g, g), _EMPTY_LO, dtype=np.int32)
    hi = np.full((g, g), _EMPTY_HI, dtype=np.int32)
    for a, b, c, t, low, high in rows:
        count[a, b] = count[b, a] = c
        total[a, b] = total[b, a] = t
        lo[a, b] = lo[b, a] = low
        hi[a, b] = hi[b, a] = high
    if groups is None:
        groups = [[name] for name in names]
    if len(groups) != g:
        raise ValueError(f"{filepath}: {g} groups in the file, {len(groups)} given")
    return names, GroupLinkage(groups, total, count, lo, hi, is_distance=is_distance)


def between_de_novo(genomes, func, groups, as_distance=True, slab_bytes=0):
    """``GroupLinkage.from_dense(matrix_de_novo(genomes, func, cpus), groups)`` -- with ``as_distance=False`` its ``inverted()``, the table
    of that matrix after ``invert()`` -- without the dense matrix: the table of the
    pair values between every two of ``groups`` -- a partition of the genomes, each group a sequence of genome names or of indices
    into ``genomes``, every genome in exactly one group -- filled on the GPU by ``Context.fill_between``: the dense matrix is never
    delivered, and beyond ``slab_bytes`` of HBM (0: automatic) never held; 24 bytes per pair of groups cross PCIe.  ``func`` must be one
    of the six ``METRICS`` callables (no CPU route: ``GroupLinkage.from_dense(matrix_de_novo(...), groups)`` serves another callable).
    Several devices as ``edges_de_novo`` (``MultiContext.fill_between``: the same table); under a launcher (``WORLD_SIZE`` > 1) it
    raises.  Every refusal comes before the first GPU call."""
    names = [g.name for g in genomes]
    members, label = _partition_labels(names, groups, "between_de_novo", BETWEEN_MAX_GROUPS)
    _, arrays = _de_novo_route(genomes, func, "between_de_novo",
        lambda ctx, metric: ctx.fill_between(metric, label, len(members), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: f"{len(genomes)} genomes in {len(members)} groups -> {len(members) * (len(members) + 1) // 2} entries from "
                                      f"{record['genome_pairs']} pairs in {stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): "
                                      f"fill+reduce+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, reduction "
                                      f"{stats.get('ms_reduce', 0.0):.3f} ms)",
        advice="for another callable: GroupLinkage.from_dense(matrix_de_novo(...), groups)")
    return GroupLinkage([[names[i] for i in idx] for idx in members], *arrays, is_distance=as_distance)


BETWEEN_VERIFY_ALONE = 256   # the smallest old group is verified alone, beyond ``verify``, up to this many members


def _verify_rows(stored_members, verify):
    """The query rows of ``between_extend``'s verification: the whole member lists (index lists) of old groups, smallest group first,
    for as long as the running total stays within ``verify`` rows; if even the smallest does not fit, that group alone when it has at
    most ``BETWEEN_VERIFY_ALONE`` members.  Returns ``(group indices verified, rows ascending)``; both empty: nothing to verify with."""
    order = sorted((len(idx), a) for a, idx in enumerate(stored_members) if idx)
    taken, total = [], 0
    for size, a in order:
        if total + size > verify:
            break
        taken.append(a)
        total += size
    if not taken and order and order[0][0] <= BETWEEN_VERIFY_ALONE:
        taken = [order[0][1]]
    return taken, sorted(i for a in taken for i in stored_members[a])


def between_extend(stored, genomes, func, groups, verify=8, slab_bytes=0):
    """``GroupLinkage.from_dense(matrix_de_novo(genomes, func, cpus), groups)`` in ``stored``'s direction, from the STORED table and the
    pairs of the new genomes alone: ``stored`` is the :class:`GroupLinkage` of an earlier collection (``between_de_novo``, or
    ``between_from_file`` with its member lists), ``groups`` the grown partition of ``genomes`` -- group i of ``stored`` a subset of
    group i, more groups may follow (the stored table is padded with empty entries for them) -- and the new genomes are those in
    ``groups`` but not in ``stored.groups``.  ``Context.fill_rows_between`` fills ``len(new) * N`` pairs instead of ``N (N - 1) / 2``
    and the result is the whole fill's, integer for integer.  The verification is exact: before the growing call ONE seedless call
    with the new genomes labelled -1 refills whole old groups, smallest first, within ``verify`` rows (``_verify_rows``; 0: none), and
    all G entries of every verified group must be the stored ones -- ValueError naming the two groups and both values otherwise.  Every
    refusal comes before the first GPU call: no partition of ``genomes``, more than ``BETWEEN_MAX_GROUPS`` groups, a stored member absent
    or moved, stored counts that are not the partition's, a launcher (``WORLD_SIZE`` > 1), a callable outside ``METRICS`` (for such a
    callable: ``GroupLinkage.extended`` over any dense matrix).  One GPU; not built: several GPUs, the launcher route, more groups,
    removing genomes."""
    if not isinstance(stored, GroupLinkage):
        raise ValueError("between_extend: stored must be a GroupLinkage")
    names = [g.name for g in genomes]
    members, label = _partition_labels(names, groups, "between_extend", BETWEEN_MAX_GROUPS)
    grown = [[names[i] for i in idx] for idx in members]
    stored._grown_members(grown, "between_extend")
    index = {name: k for k, name in enumerate(names)}
    stored_members = [sorted(index[name] for name in group) for group in stored.groups] + [[] for _ in range(len(members) - len(stored))]
    old = np.array([len(idx) for idx in stored_members], dtype=np.int64)
    seed = stored.padded(len(members))
    want = np.outer(old, old)
    np.fill_diagonal(want, old * (old - 1) // 2)
    if not np.array_equal(seed[1], want):
        a, b = (int(x) for x in np.argwhere(seed[1] != want)[0])
        raise ValueError(f"between_extend: the stored table counts {int(seed[1][a, b])} pairs between groups {a} and {b}, their {int(old[a])} and "
                         f"{int(old[b])} stored members make {int(want[a, b])}: the table is of another partition or another genome set")
    is_old = np.zeros(len(names), dtype=bool)
    for idx in stored_members:
        is_old[idx] = True
    new_idx = np.flatnonzero(~is_old).astype(np.int32)
    if new_idx.shape[0] == 0:                                              # nothing new: the stored table re-laid, no GPU call
        return GroupLinkage(grown, *seed, is_distance=stored.is_distance)
    checked, rows = _verify_rows(stored_members, max(0, int(verify)))
    if int(verify) > 0 and not checked and old.sum():
        logging.warning(f"between_extend: the smallest stored group has more than {BETWEEN_VERIFY_ALONE} members and verify is {int(verify)}: "
                        "the stored table is not verified")

    def fill(ctx, metric):
        if int(verify) > 0 and checked:
            masked = label.copy()
            masked[new_idx] = -1
            found = ctx.fill_rows_between(metric, masked, rows, len(members), as_distance=stored.is_distance, slab_bytes=slab_bytes)
            for a in checked:
                for arr, ref, what in zip(found, seed, ("sum", "count", "lo", "hi")):
                    if not np.array_equal(arr[a], ref[a]):
                        b = int(np.flatnonzero(arr[a] != ref[a])[0])
                        raise ValueError(f"between_extend: groups {a} and {b}: the stored table holds {what} {int(ref[a, b])}, the {metric} fill gives "
                                         f"{int(arr[a, b])}: the file was not written with this metric from these genomes")
        return ctx.fill_rows_between(metric, label, new_idx, len(members), seed=seed, as_distance=stored.is_distance, slab_bytes=slab_bytes,
                                     want_stats=True)

    _, arrays = _de_novo_route(genomes, func, "between_extend", fill,
        lambda stats, record, fill_s: f"{len(genomes)} genomes in {len(members)} groups, {new_idx.shape[0]} of them new ({len(rows)} old verified) -> "
                                      f"{len(members) * (len(members) + 1) // 2} entries from {int(stats['n_pairs'])} pairs in {stats['n_slabs']} slab(s): "
                                      f"fill+reduce+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, reduction "
                                      f"{stats.get('ms_reduce', 0.0):.3f} ms)",
        advice="for another callable: GroupLinkage.extended over any dense matrix", several=False)
    LAST_FILL.update(rows=int(new_idx.shape[0]), verified_rows=len(rows))
    return GroupLinkage(grown, *arrays, is_distance=stored.is_distance)
