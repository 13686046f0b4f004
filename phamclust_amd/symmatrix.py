"""``SymMatrix``: the reference's symmetric matrix (matrix.py:33-405) over ndarray storage.

It keeps the reference's method surface but stores a dense float64 array (NaN = unset) plus a name -> slot map instead of a
dict of dicts, so the downstream clustering step gets its ndarray without N^2 Python calls.  Behaviour kept on purpose: weights
are rounded to 6 places and range-checked on write (matrix.py:316-323), ``__iter__`` yields the upper half incl. the diagonal
in current node order (matrix.py:368-379), ``medoid`` counts the diagonal twice and breaks ties by node order
(matrix.py:80-104), ``lock()`` makes writes fail (matrix.py:308-309).

Owns ``SymMatrix``, ``_square_matrix`` (a matrix around a ready array) and ``_get_tree_order`` (what ``reorder`` sorts by).
The bottom of the package's matrix modules: it imports nothing of the project but ``statistics``.
"""

import numpy as np
from scipy.cluster.hierarchy import dendrogram, linkage
from scipy.spatial.distance import squareform

from phamclust_amd.statistics import average, skewness, standard_deviation


class SymMatrix:
    def __init__(self, nodes, is_distance=False):
        self._nodes = nodes
        self._slot = {name: k for k, name in enumerate(nodes)}
        n = len(nodes)
        self._data = np.full((n, n), np.nan, dtype=np.float64)
        self._is_distance = is_distance
        self._locked = False

    # -- bulk constructors (new; used by the GPU fill) -----------------------------
    @classmethod
    def from_condensed(cls, nodes, condensed, is_distance=True):
        """Build from a scipy-condensed vector whose values are already rounded to 6 places;
        the diagonal is preset to ``1.0 - is_distance`` as matrix_de_novo does (matrix.py:467-468)."""
        nodes = list(nodes)
        n = len(nodes)
        condensed = np.ascontiguousarray(condensed, dtype=np.float64)
        if condensed.shape != (n * (n - 1) // 2,):
            raise ValueError(f"need {n * (n - 1) // 2} condensed values but got {condensed.shape}")
        if condensed.size and not (np.nanmin(condensed) >= 0.0 and np.nanmax(condensed) <= 1.0):
            raise ValueError("weight not in [0.0, 1.0]")
        self = cls.__new__(cls)
        self._nodes = nodes
        self._slot = {name: k for k, name in enumerate(nodes)}
        # scipy expands the vector in C: no N^2/2 index arrays (two of them were 800 MB at N = 10,000)
        self._data = squareform(condensed, force="tomatrix", checks=False) if n > 1 else np.zeros((n, n), dtype=np.float64)
        self._is_distance = is_distance
        self._locked = False
        if not is_distance:
            np.fill_diagonal(self._data, 1.0)
        return self

    # -- properties ------------------------------------------------------------------
    @property
    def is_distance(self):
        return self._is_distance

    @property
    def nodes(self):
        return self._nodes[:]

    def _order(self):
        return np.fromiter((self._slot[name] for name in self._nodes), dtype=np.int64, count=len(self._nodes))

    def _ordered(self):
        """The weights in current node order.  READ-ONLY for callers: when the traversal order is still the storage
        order this is the storage itself, not a copy (an N = 10,000 matrix is 800 MB)."""
        order = self._order()
        if order.size == self._data.shape[0] and (order == np.arange(order.size)).all():
            return self._data
        return self._data[np.ix_(order, order)]

    @property
    def diameter(self):
        if not self.is_distance:
            raise ValueError("cannot compute diameter for similarity matrix")
        n = len(self)
        if n < 2:
            return 0.0
        off = squareform(self._ordered(), force="tovector", checks=False)
        top = np.nanmax(off) if off.size else 0.0
        return round(float(max(top, 0.0)), 6)

    def _central(self):
        """Per node, the mean of its N+1 incident weights.  The reference gathers them by walking the upper half
        (matrix.py:84-97), so node k's list reads w(0,k) .. w(k-1,k), w(k,k) TWICE, w(k,k+1) .. and is summed left
        to right; sweeping the columns in order and adding the diagonal a second time right after its own column
        adds the same numbers in the same order for every node at once (ties between nodes fall as they do there)."""
        n = len(self)
        m = self._ordered()
        totals = np.zeros(n, dtype=np.float64)
        for j in range(n):
            totals += m[j]                       # column j == row j (symmetric); contiguous
            totals[j] += m[j, j]
        return [(name, float(total) / (n + 1)) for name, total in zip(self._nodes, totals)]

    @property
    def medoid(self):
        scored = sorted(self._central(), key=lambda item: item[1])
        return scored[0] if self.is_distance else scored[-1]

    @property
    def anti_medoid(self):
        scored = sorted(self._central(), key=lambda item: item[1])
        return scored[-1] if self.is_distance else scored[0]

    @property
    def statistics(self):
        if len(self) == 1:
            node = self._nodes[0]
            return self.get_weight(node, node), 0.0, 0.0
        edges = squareform(self._ordered(), force="tovector", checks=False).tolist()    # upper half, row by row
        mean = average(edges)
        std_dev = standard_deviation(edges, mean)
        skew = 0.0 if std_dev == 0.0 else skewness(edges, mean)
        return mean, std_dev, skew

    # -- structure -------------------------------------------------------------------
    def extract_submatrix(self, nodes):
        for name in nodes:
            if name not in self:
                raise KeyError(f"node '{name}' not in matrix")
        sub = SymMatrix(nodes, self.is_distance)
        idx = np.fromiter((self._slot[name] for name in nodes), dtype=np.int64, count=len(nodes))
        sub._data = self._data[np.ix_(idx, idx)].copy()
        return sub

    def append_node(self, source, data):
        """Grow by one node whose weights to every node (itself included) come in ``data`` (matrix.py:169-213):
        the new name must be new, ``data`` must cover exactly the current nodes plus the new one, and the self-edge
        must be what the diagonal of this kind of matrix holds."""
        if self._locked:
            raise AttributeError("matrix is marked as read-only")
        if source in self:
            raise KeyError(f"node '{source}' is already in this matrix")
        if source not in data:
            raise KeyError(f"incoming data lacks an self-edge for '{source}'")
        on_diagonal = 0.0 if self.is_distance else 1.0
        if data[source] != on_diagonal:
            kind = "distance" if self.is_distance else "similarity"
            raise ValueError(f"nonsense value {data[source]} for self-edge on {kind} matrix")
        given = set(data) - {source}
        absent = set(self._slot) - given
        if absent:
            raise KeyError(f"missing edge(s) for {source} vs: {absent}")
        unknown = given - set(self._slot)
        if unknown:
            raise KeyError(f"specified edges for nodes not found in matrix: {unknown}")
        n = self._data.shape[0]
        edge = np.empty(n + 1, dtype=np.float64)
        for name, k in self._slot.items():
            edge[k] = data[name]
        edge[n] = data[source]
        if not (edge.min() >= 0.0 and edge.max() <= 1.0):
            raise ValueError(f"weight {edge[(edge < 0.0) | (edge > 1.0) | (edge != edge)][0]} not in [0.0, 1.0]")
        edge = np.array([round(float(w), 6) for w in edge])     # Python's round: what set_weight stores (matrix.py:323)
        grown = np.empty((n + 1, n + 1), dtype=np.float64)
        grown[:n, :n] = self._data
        grown[n, :] = edge
        grown[:, n] = edge
        self._data = grown
        self._slot[source] = n
        self._nodes.append(source)

    def get_weight(self, source, target):
        if source not in self:
            raise KeyError(f"node '{source}' not in matrix")
        if target not in self:
            raise KeyError(f"node '{target}' not in matrix")
        value = self._data[self._slot[source], self._slot[target]]
        return None if value != value else float(value)

    def set_weight(self, source, target, weight):
        if self._locked:
            raise AttributeError("matrix is marked as read-only")
        if source not in self:
            raise KeyError(f"node '{source}' not in matrix")
        if target not in self:
            raise KeyError(f"node '{target}' not in matrix")
        if not 0 <= weight <= 1:
            raise ValueError(f"weight {weight} not in [0.0, 1.0]")
        i, j = self._slot[source], self._slot[target]
        self._data[i, j] = self._data[j, i] = round(weight, 6)

    def invert(self):
        """distance <-> similarity in place: every stored w becomes round(1 - w, 6)
        (matrix.py:236-247).  Stored values are 6-place decimals, so numpy's rounding and
        Python's agree here."""
        if self._locked:
            raise AttributeError("matrix is marked as read-only")
        self._data = np.round(1.0 - self._data, 6)
        self._is_distance = not self.is_distance
        return self

    def reorder(self, nodes=None):
        """New traversal order (storage stays put); without ``nodes``: leaf order of the single-linkage tree
        (matrix.py:249-263)."""
        order = list(nodes) if nodes else [self._nodes[leaf] for leaf in _get_tree_order(self)]
        if len(order) != len(self._nodes):
            raise ValueError(f"need {len(self)} nodes but got {len(order)}")
        stranger = next((name for name in order if name not in self), None)
        if stranger is not None:
            raise KeyError(f"node '{stranger}' not in matrix")
        self._nodes = order

    def nearest_neighbors(self, source, threshold):
        """Nodes within ``threshold`` of ``source`` (<= on distances, >= on similarities), closest first; equally
        close ones keep their traversal order (matrix.py:265-296: a stable sort, reversed for similarities)."""
        order = self._order()
        if order.size == 0 or (order.size == 1 and self._nodes[0] == source):
            return []
        if source not in self:
            raise KeyError(f"node '{source}' not in matrix")
        row = self._data[self._slot[source], order]
        others = order != self._slot[source]
        if np.isnan(row[others]).any():
            raise TypeError("cannot rank neighbours of a node with unset edges")
        near = np.flatnonzero(others & ((row <= threshold) if self.is_distance else (row >= threshold)))
        ranked = near[np.argsort(row[near] if self.is_distance else -row[near], kind="stable")]
        return [self._nodes[k] for k in ranked]

    def lock(self):
        self._locked = True

    def unlock(self):
        self._locked = False

    def is_locked(self):
        return self._locked

    def to_ndarray(self, condensed=False):
        full = self._ordered()
        if condensed:
            return squareform(full, force="tovector")
        return full.copy() if full is self._data else full

    # -- container protocol ------------------------------------------------------------
    def __contains__(self, item):
        if not isinstance(item, str):
            raise TypeError(f"type(item) should be 'str', not '{type(item)}'")
        return item in self._slot

    def __getitem__(self, item):
        """Row of ``item`` as the reference stores it: only targets that do not sort before
        ``item`` as strings (matrix.py:231-232, 320-321)."""
        if item not in self:
            raise KeyError(f"node '{item}' not in matrix")
        row = self._data[self._slot[item]]
        return {name: float(row[k]) for name, k in self._slot.items() if not name < item and row[k] == row[k]}

    def __iter__(self):
        m = self._ordered()
        for i, source in enumerate(self._nodes):
            row = m[i]
            for j in range(i, len(self._nodes)):
                value = row[j]
                yield source, self._nodes[j], (None if value != value else float(value))

    def iterrows(self):
        m = self._ordered()
        for i, source in enumerate(self._nodes):
            yield source, [None if v != v else v for v in m[i].tolist()]

    def __len__(self):
        return len(self._nodes)

    def __lt__(self, other):
        if not isinstance(other, SymMatrix):
            raise TypeError(f"cannot compare SymMatrix to {type(other)}")
        return len(self) < len(other)

    def __str__(self):
        lines = [f"{len(self)}\n"]
        for source, row in self.iterrows():
            lines.append(f"{source:<24}\t" + "\t".join([f"{x:.6f}" for x in row]) + "\n")
        return "".join(lines)


def _square_matrix(nodes, data, is_distance):
    """A SymMatrix over ``nodes`` that takes ``data`` (N x N, already rounded, diagonal set) as its storage."""
    m = SymMatrix.__new__(SymMatrix)
    m._nodes = list(nodes)
    m._slot = {name: k for k, name in enumerate(m._nodes)}
    m._data = data
    m._is_distance = is_distance
    m._locked = False
    return m


def _get_tree_order(matrix):
    """Leaf order of a single-linkage dendrogram on distances (matrix.py:673-686)."""
    if not matrix.is_distance:
        matrix = matrix.extract_submatrix(matrix.nodes)
        matrix.invert()
    z = linkage(matrix.to_ndarray(condensed=True), method="single")
    return dendrogram(z, no_plot=True, get_leaves=True, count_sort="descending")["leaves"]
