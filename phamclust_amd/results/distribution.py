"""``PairDistribution``: the exact distribution of a collection's pair values, and the routes that fill it without the dense matrix.

Every delivered value is ``round(x, 6)``, one of the 10^6 + 1 millionths in [0, 1], so the whole distribution of N (N - 1) / 2 values
is an integer histogram of ``HIST_BINS`` bins, whatever N is.  From it follow, exactly and for every threshold at once, the count of
pairs within a threshold (what ``edges_de_novo`` would deliver, before it is asked for), every quantile, and the mean, standard
deviation and skewness ``SymMatrix.statistics`` takes from the dense matrix.  Split by a partition into the pairs inside a group
("within") and between two ("between") it shows how well a threshold separates the clusters.

Owns ``PairDistribution``, ``distribution_de_novo`` (``Context.fill_hist`` / ``MultiContext.fill_hist``), ``distribution_extend``
(``Context.fill_rows_hist``) and the file pair ``distribution_to_file`` / ``distribution_from_file``.  All statistics are computed from
Python integers and ``fractions`` and converted to float once: nothing is accumulated in floating point.
"""

import math
from fractions import Fraction

import numpy as np

from phamclust_amd.results._common import _live_row_pairs, _passes
from phamclust_amd.routes import _de_novo_route, _extend_fill, _extend_plan, _partition_labels

HIST_BINS = 1000001
MILLION = 1000000


def _micro_of(values, caller):
    """``values`` as millionths (int64): ValueError for one that is no millionth in [0, 1] (-0.0 is the millionth 0)."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    k = np.rint(values * 1.0e6)
    ok = (k >= 0) & (k <= MILLION)
    ok &= np.where(ok, k, 0.0) / 1.0e6 == values
    if not ok.all():
        at = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"{caller}: value {values[at]!r} is no millionth in [0, 1]")
    return k.astype(np.int64)


def _bins_of(micro):
    """The non-empty bins ``(micro ascending, count)`` of an int64 array of millionths."""
    if micro.size == 0:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
    dense = np.bincount(micro, minlength=HIST_BINS)
    at = np.flatnonzero(dense)
    return at.astype(np.int64), dense[at].astype(np.int64)


def _add_bins(a, b):
    dense = np.zeros(HIST_BINS, dtype=np.int64)
    np.add.at(dense, a[0], a[1])
    np.add.at(dense, b[0], b[1])
    at = np.flatnonzero(dense)
    return at.astype(np.int64), dense[at]


class PairDistribution:
    """The histogram of pair values: per class the non-empty bins ``(micro, count)`` -- ``micro`` ascending int64 millionths,
    ``count`` positive int64.  One class (``bins`` a single pair of arrays), or two when a partition split the pairs: ``bins =
    [(micro, count) within, (micro, count) between]``.  ``is_distance`` says what the values are.  ``nodes``: the genome names the
    distribution covers, when known (``distribution_extend`` needs them: a histogram cannot name its pairs)."""

    def __init__(self, bins, is_distance=True, nodes=None):
        if len(bins) == 2 and (len(bins[0]) == 0 or np.ndim(bins[0][0]) == 0):       # one (micro, count), not two classes
            bins = [bins]
        bins = list(bins)
        if len(bins) not in (1, 2):
            raise ValueError(f"PairDistribution: {len(bins)} classes (1, or 2: within and between)")
        self._bins = []
        for micro, count in bins:
            micro = np.ascontiguousarray(micro, dtype=np.int64).reshape(-1)
            count = np.ascontiguousarray(count, dtype=np.int64).reshape(-1)
            if micro.shape != count.shape:
                raise ValueError(f"PairDistribution: {micro.shape[0]} bins and {count.shape[0]} counts")
            if micro.size and (micro.min() < 0 or micro.max() > MILLION):
                raise ValueError("PairDistribution: a bin outside [0, 10^6]")
            if micro.size > 1 and not (np.diff(micro) > 0).all():
                raise ValueError("PairDistribution: the bins must be strictly ascending")
            if (count < 0).any():
                raise ValueError(f"PairDistribution: bin {int(micro[np.flatnonzero(count < 0)[0]])} has a negative count")
            keep = count > 0
            self._bins.append((micro[keep], count[keep]))
        self.is_distance = bool(is_distance)
        self.nodes = list(nodes) if nodes is not None else None

    # -- constructors -----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_hist(cls, hist, is_distance=True, nodes=None):
        """From the dense array ``Context.fill_hist`` delivers: int64 ``[1 or 2, HIST_BINS]``."""
        hist = np.asarray(hist)
        if hist.ndim != 2 or hist.shape[0] not in (1, 2) or hist.shape[1] != HIST_BINS:
            raise ValueError(f"PairDistribution.from_hist: an array [1 or 2, {HIST_BINS}], not {hist.shape}")
        bins = []
        for row in hist:
            at = np.flatnonzero(row)
            bins.append((at.astype(np.int64), np.asarray(row[at], dtype=np.int64)))
        return cls(bins, is_distance=is_distance, nodes=nodes)

    @classmethod
    def from_dense(cls, matrix, groups=None):
        """The host statement for any ``SymMatrix``: the histogram of its N (N - 1) / 2 off-diagonal values, in its direction;
        ``groups`` (a partition of its nodes: lists of names or of indices) splits it into within and between."""
        nodes = matrix.nodes
        n = len(nodes)
        data = np.asarray(matrix._ordered(), dtype=np.float64)
        s, t = np.triu_indices(n, k=1)
        micro = _micro_of(data[s, t], "PairDistribution.from_dense")
        if groups is None:
            return cls([_bins_of(micro)], is_distance=matrix.is_distance, nodes=nodes)
        _, label = _partition_labels(nodes, groups, "PairDistribution.from_dense", max(n, 1))
        same = label[s] == label[t]
        return cls([_bins_of(micro[same]), _bins_of(micro[~same])], is_distance=matrix.is_distance, nodes=nodes)

    # -- shape ------------------------------------------------------------------------------------------------------------------
    @property
    def n_classes(self):
        return len(self._bins)

    @property
    def partitioned(self):
        return len(self._bins) == 2

    def _need_partition(self, what):
        if not self.partitioned:
            raise ValueError(f"PairDistribution.{what}: the distribution is not split by a partition")

    @property
    def within(self):
        self._need_partition("within")
        return PairDistribution([self._bins[0]], is_distance=self.is_distance, nodes=self.nodes)

    @property
    def between(self):
        self._need_partition("between")
        return PairDistribution([self._bins[1]], is_distance=self.is_distance, nodes=self.nodes)

    @property
    def whole(self):
        """The distribution of all pairs, the partition forgotten."""
        return PairDistribution([self._merged()], is_distance=self.is_distance, nodes=self.nodes)

    def _merged(self):
        return self._bins[0] if len(self._bins) == 1 else _add_bins(*self._bins)

    @property
    def micro(self):
        """The non-empty bins of all pairs, ascending millionths."""
        return self._merged()[0]

    @property
    def count(self):
        return self._merged()[1]

    def bins(self, cls=None):
        """``(micro, count)`` of class ``cls`` (0: within, 1: between), or of all pairs."""
        return self._merged() if cls is None else self._bins[cls]

    def to_hist(self):
        """The dense int64 array ``[n_classes, HIST_BINS]`` (what ``Context.fill_rows_hist`` takes as its seed)."""
        hist = np.zeros((len(self._bins), HIST_BINS), dtype=np.int64)
        for row, (micro, count) in zip(hist, self._bins):
            row[micro] = count
        return hist

    def inverted(self):
        """The distribution of the inverted matrix: every millionth's complement, the direction flipped."""
        return PairDistribution([((MILLION - micro)[::-1], count[::-1]) for micro, count in self._bins], is_distance=not self.is_distance, nodes=self.nodes)

    def __eq__(self, other):
        return (isinstance(other, PairDistribution) and self.is_distance == other.is_distance and len(self._bins) == len(other._bins)
                and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(self._bins, other._bins)))

    __hash__ = None

    def __add__(self, other):
        """Bin by bin: the distribution of two disjoint sets of pairs."""
        if not isinstance(other, PairDistribution):
            return NotImplemented
        if self.is_distance != other.is_distance or len(self._bins) != len(other._bins):
            raise ValueError("PairDistribution: the two distributions differ in direction or in their classes")
        return PairDistribution([_add_bins(a, b) for a, b in zip(self._bins, other._bins)], is_distance=self.is_distance)

    def extended(self, n, rows, values, labels=None, nodes=None):
        """The host statement of the rows form: this distribution -- of the pairs among the genomes that are not in ``rows`` --
        grown by the pairs of a rows array, ``values[i, g]`` the pair {rows[i], g} of ``n`` genomes, each once (the diagonal is
        none; a pair of two rows is the smaller one's).  ``labels`` (int, ``[n]``) is needed when the distribution is split."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        src, tgt, w = _live_row_pairs(int(n), rows, values)
        micro = _micro_of(w, "PairDistribution.extended")
        if not self.partitioned:
            if labels is not None:
                raise ValueError("PairDistribution.extended: labels for a distribution that is not split")
            grown = [_bins_of(micro)]
        else:
            if labels is None:
                raise ValueError("PairDistribution.extended: a split distribution needs the genomes' labels")
            labels = np.asarray(labels).reshape(-1)
            if labels.shape[0] != int(n):
                raise ValueError(f"PairDistribution.extended: {labels.shape[0]} labels for {int(n)} genomes")
            same = labels[src] == labels[tgt]
            grown = [_bins_of(micro[same]), _bins_of(micro[~same])]
        out = self + PairDistribution(grown, is_distance=self.is_distance)
        out.nodes = list(nodes) if nodes is not None else None
        return out

    def check_seed(self, n_old, old_labels=None, caller="PairDistribution.check_seed"):
        """What the rows form refuses of a seed, stated on the host: the total must be the ``n_old (n_old - 1) / 2`` pairs of the
        old genomes, and with a partition class 0 their within count (``old_labels``: the old genomes' labels).  Necessary, not
        sufficient: a histogram cannot name its pairs."""
        n_old = int(n_old)
        want = n_old * (n_old - 1) // 2
        if self.n_pairs != want:
            raise ValueError(f"{caller}: the stored distribution counts {self.n_pairs} pairs, the {n_old} stored genomes have {want}: "
                             "it is of another genome set")
        if self.partitioned:
            if old_labels is None:
                raise ValueError(f"{caller}: a split distribution needs the partition")
            sizes = np.bincount(np.asarray(old_labels, dtype=np.int64).reshape(-1)) if n_old else np.zeros(1, dtype=np.int64)
            within = int(sum(int(c) * (int(c) - 1) // 2 for c in sizes))
            if int(self._bins[0][1].sum()) != within:
                raise ValueError(f"{caller}: the stored distribution counts {int(self._bins[0][1].sum())} pairs inside the groups, the partition "
                                 f"has {within} over the stored genomes: it is of another partition or another genome set")
        elif old_labels is not None:
            raise ValueError(f"{caller}: a partition for a distribution that is not split")

    # -- exact statistics -------------------------------------------------------------------------------------------------------
    @property
    def n_pairs(self):
        return int(sum(int(count.sum()) for _, count in self._bins))

    def _need_pairs(self, what):
        if self.n_pairs == 0:
            raise ValueError(f"PairDistribution.{what}: no pairs")

    @property
    def min(self):
        self._need_pairs("min")
        return int(self.micro[0]) / 1.0e6

    @property
    def max(self):
        self._need_pairs("max")
        return int(self.micro[-1]) / 1.0e6

    def _power_sums(self):
        """(n, sum k, sum k^2, sum k^3) over all pairs, k in millionths: Python integers (sum k^3 passes 2^64 at N of a few thousand)."""
        micro, count = self._merged()
        ks, cs = [int(k) for k in micro], [int(c) for c in count]
        return (sum(cs), sum(c * k for k, c in zip(ks, cs)), sum(c * k * k for k, c in zip(ks, cs)), sum(c * k * k * k for k, c in zip(ks, cs)))

    def _moments(self):
        """(n, mean, sum (v - mean)^2, sum (v - mean)^3) as exact rationals, v = k / 10^6."""
        n, s1, s2, s3 = self._power_sums()
        mean = Fraction(s1, n)
        q2 = Fraction(s2) - mean * s1
        q3 = Fraction(s3) - 3 * mean * s2 + 3 * mean * mean * s1 - n * mean ** 3
        return n, mean / MILLION, q2 / MILLION ** 2, q3 / MILLION ** 3

    @property
    def mean(self):
        self._need_pairs("mean")
        return float(self._moments()[1])

    def variance_exact(self, sample=True):
        """The variance as a ``Fraction``; 0 for a single pair, as the reference's ``variance``."""
        self._need_pairs("variance")
        n, _, q2, _ = self._moments()
        return Fraction(0) if n == 1 else q2 / (n - 1 if sample else n)

    def std_dev(self, sample=True):
        """The square root of the exact variance converted once."""
        return math.sqrt(float(self.variance_exact(sample)))

    def skewness_squared_exact(self, sample=True):
        """``(sign, skewness^2)``, the square an exact ``Fraction`` (the skewness itself is irrational): the reference's form, sum (v -
        mean)^3 / ((n - 1) s^3) with the sample deviation s (``sample=False``: n and the population deviation); (0, 0) when the
        deviation is 0 or there is a single pair."""
        self._need_pairs("skewness")
        n, _, q2, q3 = self._moments()
        if n == 1 or q2 == 0:
            return 0, Fraction(0)
        d = n - 1 if sample else n
        return (q3 > 0) - (q3 < 0), q3 * q3 / (d * d * (q2 / d) ** 3)

    def skewness(self, sample=True):
        sign, square = self.skewness_squared_exact(sample)
        return sign * math.sqrt(float(square))

    @property
    def statistics(self):
        """``SymMatrix.statistics``' triple -- mean, sample standard deviation, sample skewness (0.0 when the deviation is 0) --
        from the exact integers."""
        std = self.std_dev()
        return self.mean, std, 0.0 if std == 0.0 else self.skewness()

    def count_within(self, threshold, strict=False, cls=None):
        """How many pairs pass ``threshold`` under the predicate of ``Context.fill_edges`` / ``fill_components``: ``<=`` on
        distances, ``>=`` on similarities; ``<`` / ``>`` with ``strict``.  ``cls``: of one class only."""
        micro, count = self.bins(cls)
        return int(count[_passes(micro / 1.0e6, float(threshold), self.is_distance, strict)].sum())

    def quantile(self, q):
        """The smallest value v with at least ``ceil(q n)`` pairs at or below it (q = 0: the minimum)."""
        self._need_pairs("quantile")
        q = Fraction(q)
        if not 0 <= q <= 1:
            raise ValueError(f"PairDistribution.quantile: q {float(q)} is outside [0, 1]")
        micro, count = self._merged()
        rank = max(1, math.ceil(q * self.n_pairs))
        return int(micro[int(np.searchsorted(np.cumsum(count), rank, side="left"))]) / 1.0e6

    @property
    def median(self):
        return self.quantile(Fraction(1, 2))

    def cumulative(self):
        """``(value, pairs)``: for every non-empty bin's value, ascending, ``count_within(value)``."""
        micro, count = self._merged()
        within = np.cumsum(count) if self.is_distance else np.cumsum(count[::-1])[::-1]
        return micro / 1.0e6, within.astype(np.int64)

    def threshold_for(self, max_pairs):
        """The loosest threshold (a millionth) whose passing pairs (``count_within``) stay within ``max_pairs``; None when even
        the tightest threshold, 0.0 on distances and 1.0 on similarities, passes more."""
        max_pairs = int(max_pairs)
        micro, count = self._merged()
        if self.is_distance:
            over = np.flatnonzero(np.cumsum(count) > max_pairs)
            if over.size == 0:
                return 1.0
            k = int(micro[over[0]]) - 1
            return None if k < 0 else k / 1.0e6
        over = np.flatnonzero(np.cumsum(count[::-1]) > max_pairs)
        if over.size == 0:
            return 0.0
        k = int(micro[::-1][over[0]]) + 1
        return None if k > MILLION else k / 1.0e6

    # -- a partition's separation -------------------------------------------------------------------------------------------------
    def separation(self, threshold, strict=False):
        """``(within pairs beyond the threshold, between pairs inside it)``: what a clustering at ``threshold`` would cut and
        would join against the partition."""
        self._need_partition("separation")
        return (int(self._bins[0][1].sum()) - self.count_within(threshold, strict, cls=0), self.count_within(threshold, strict, cls=1))

    def best_separation(self):
        """``(threshold, within beyond, between inside)`` of the millionth that minimises their sum; the smallest such threshold
        on ties."""
        self._need_partition("best_separation")
        dense = self.to_hist()
        w, b = dense[0], dense[1]
        if self.is_distance:
            beyond = int(w.sum()) - np.cumsum(w)
            inside = np.cumsum(b)
        else:
            beyond = np.concatenate(([0], np.cumsum(w)[:-1]))
            inside = np.cumsum(b[::-1])[::-1]
        k = int(np.argmin(beyond + inside))
        return k / 1.0e6, int(beyond[k]), int(inside[k])

    # -- files ------------------------------------------------------------------------------------------------------------------
    def to_file(self, filepath):
        """A TSV of the non-empty bins, ascending: ``value<TAB>count``, or ``value<TAB>within<TAB>between`` when split."""
        with open(filepath, "w") as handle:
            if not self.partitioned:
                handle.write("value\tcount\n")
                handle.writelines(f"{int(k) / 1.0e6:.6f}\t{int(c)}\n" for k, c in zip(*self._bins[0]))
            else:
                dense = self.to_hist()
                handle.write("value\twithin\tbetween\n")
                handle.writelines(f"{int(k) / 1.0e6:.6f}\t{int(dense[0, k])}\t{int(dense[1, k])}\n" for k in np.flatnonzero(dense[0] + dense[1]))
        return filepath

    @classmethod
    def from_file(cls, filepath, is_distance=True, nodes=None):
        """The distribution a file of ``to_file`` holds, bin for bin; ``is_distance``: what the file's values are.  ValueError for
        a file that is none."""
        with open(filepath, "r") as handle:
            header = next(handle, "").rstrip("\n").split("\t")
            if header not in (["value", "count"], ["value", "within", "between"]):
                raise ValueError(f"{filepath}: no distribution file (header {header})")
            classes = len(header) - 1
            micro, counts = [], [[] for _ in range(classes)]
            for number, line in enumerate(handle, start=2):
                fields = line.rstrip("\n").split("\t")
                if len(fields) != classes + 1:
                    raise ValueError(f"{filepath}:{number}: expected {classes + 1} columns")
                try:
                    k = int(np.rint(float(fields[0]) * 1.0e6))
                    row = [int(x) for x in fields[1:]]
                except ValueError:
                    raise ValueError(f"{filepath}:{number}: no bin") from None
                if not 0 <= k <= MILLION or (micro and k <= micro[-1]) or min(row) < 0:
                    raise ValueError(f"{filepath}:{number}: bins must ascend within [0, 1] and counts must not be negative")
                micro.append(k)
                for col, x in zip(counts, row):
                    col.append(x)
        return cls([(micro, col) for col in counts], is_distance=is_distance, nodes=nodes)


def distribution_to_file(distribution, filepath):
    return distribution.to_file(filepath)


def distribution_from_file(filepath, is_distance=True, nodes=None):
    return PairDistribution.from_file(filepath, is_distance=is_distance, nodes=nodes)


def _labels_of(names, groups, caller):
    """``(label array or None, number of groups)`` of an optional partition (no cap on the groups: labels are only compared)."""
    if groups is None:
        return None, 0
    members, label = _partition_labels(names, groups, caller, max(len(names), 1))
    return label, len(members)


def distribution_de_novo(genomes, func, groups=None, as_distance=True, slab_bytes=0):
    """``PairDistribution.from_dense(matrix_de_novo(genomes, func, cpus), groups)`` -- with ``as_distance=False`` its ``inverted()`` --
    without the dense matrix: ``Context.fill_hist`` counts every filled slab into a histogram that stays on the device, and 8 MB per
    class cross PCIe at the end.  ``groups``: a partition of the genomes (lists of names or of indices into ``genomes``, every genome
    in exactly one), which splits the distribution into within and between.  ``func`` must be one of the six ``METRICS`` callables
    (for another: ``PairDistribution.from_dense`` over any dense matrix).  Several devices as ``edges_de_novo``
    (``MultiContext.fill_hist``: the same histogram); under a launcher (``WORLD_SIZE`` > 1) it raises.  Every refusal comes before
    the first GPU call."""
    names = [g.name for g in genomes]
    label, n_groups = _labels_of(names, groups, "distribution_de_novo")
    _, arrays = _de_novo_route(genomes, func, "distribution_de_novo",
        lambda ctx, metric: ctx.fill_hist(metric, label, n_groups or None, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: f"{len(genomes)} genomes -> {stats['n_classes']} x {HIST_BINS} bins from {record['genome_pairs']} pairs in "
                                      f"{stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): fill+count+D2H {fill_s:.3f} s (kernels "
                                      f"{stats['ms_total']:.3f} ms, passes {stats.get('ms_pass', 0.0):.3f} ms)",
        advice="for another callable: PairDistribution.from_dense(matrix_de_novo(...), groups)")
    return PairDistribution.from_hist(arrays[0], is_distance=as_distance, nodes=names)


def distribution_extend(stored, genomes, func, groups=None, verify=4, slab_bytes=0):
    """``PairDistribution.from_dense(matrix_de_novo(genomes, func, cpus), groups)`` in ``stored``'s direction, from the STORED
    distribution and the pairs of the new genomes alone: ``stored`` is the :class:`PairDistribution` of an earlier collection with
    its ``nodes`` (``distribution_de_novo``, or ``distribution_from_file(..., nodes=...)``), the new genomes are those of ``genomes``
    it lacks, and ``Context.fill_rows_hist`` counts ``len(new) * N`` pairs instead of ``N (N - 1) / 2``.  ``groups``: the grown
    partition, needed exactly when ``stored`` is split.  The guard: the rows of ``verify`` old genomes are refilled, every value of
    an old-old pair in them must fall in a bin ``stored`` populates (in its class, when split), and the stored total must be
    ``N_old (N_old - 1) / 2`` (split: class 0 the old genomes' within count) -- ValueError naming the pair otherwise.  That check is
    NECESSARY, NOT SUFFICIENT: a histogram cannot name its pairs, so a stale file whose values happen to fall in populated bins
    passes.  Refusals and routes as ``tree_extend``; one GPU."""
    if not isinstance(stored, PairDistribution):
        raise ValueError("distribution_extend: stored must be a PairDistribution")
    if stored.nodes is None:
        raise ValueError("distribution_extend: the stored distribution does not know its genomes (PairDistribution.nodes; "
                         "distribution_from_file takes them as nodes=)")
    if stored.partitioned != (groups is not None):
        raise ValueError("distribution_extend: groups is needed exactly when the stored distribution is split by a partition")
    plan = names, old_at, new_idx = _extend_plan(stored.nodes, genomes, "distribution_extend")
    as_distance = stored.is_distance
    if old_at.shape[0] == 0:
        return distribution_de_novo(genomes, func, groups=groups, as_distance=as_distance, slab_bytes=slab_bytes)
    label, n_groups = _labels_of(names, groups, "distribution_extend")
    stored.check_seed(old_at.shape[0], None if label is None else label[old_at], "distribution_extend")
    if not new_idx:
        return PairDistribution(stored._bins, is_distance=as_distance, nodes=names)
    as_dist = stored if as_distance else stored.inverted()                 # (the guard refills distances: a similarity FILL's values differ at a tie)
    populated = as_dist.to_hist() > 0
    is_old = np.zeros(len(names), dtype=bool)
    is_old[old_at] = True

    def guard(metric, checked, values):
        for q, row in zip(checked, values):
            others = np.flatnonzero(is_old)
            others = others[others != q]
            micro = _micro_of(row[others], "distribution_extend")
            cls = (label[others] != label[q]).astype(np.int64) if label is not None else np.zeros(others.shape[0], dtype=np.int64)
            miss = np.flatnonzero(~populated[cls, micro])
            if miss.size:
                g = int(others[miss[0]])
                raise ValueError(f"distribution_extend: pair ('{names[min(q, g)]}', '{names[max(q, g)]}'): the {metric} fill gives distance "
                                 f"{int(micro[miss[0]]) / 1.0e6:.6f}, a value the stored distribution does not hold: it was not made with this "
                                 "metric from these genomes")

    arrays = _extend_fill(plan, genomes, func, "distribution_extend", True, verify, guard,
        lambda ctx, metric: ctx.fill_rows_hist(metric, new_idx, group=label, n_groups=n_groups or None, seed=stored.to_hist(), as_distance=as_distance,
                                               slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: (
            f"{len(new_idx)} new of {len(names)} genomes -> {stats['n_pairs']} pairs counted in {stats['n_slabs']} slab(s): guard+fill+count+D2H "
            f"{fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, passes {stats.get('ms_pass', 0.0):.3f} ms)"))
    return PairDistribution.from_hist(arrays[0], is_distance=as_distance, nodes=names)
