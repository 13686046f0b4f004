"""``SymMatrix`` and ``matrix_de_novo``: the reference's matrix.py surface over ndarray storage.

``matrix_de_novo(genomes, func, cpus, as_distance=True)`` is the drop-in boundary
(reference matrix.py:432-497, called from scripts/phamclust.py:258).  When ``func`` is one
of the six ``METRICS`` callables the whole N x N fill runs on the GPU through
``libphamclust_hip.so`` (one upload, one ``pc_fill``); any other callable takes the generic
per-pair loop with the reference's semantics.  There is no CPU fallback for the six
metrics: a missing library or a failing call raises.

``SymMatrix`` keeps the reference's method surface (matrix.py:33-405) but stores a dense
float64 array (NaN = unset) plus a name -> slot map instead of a dict of dicts, so the
downstream clustering step gets its ndarray without N^2 Python calls.  Behaviour kept on
purpose: weights are rounded to 6 places and range-checked on write (matrix.py:316-323),
``__iter__`` yields the upper half incl. the diagonal in current node order
(matrix.py:368-379), ``medoid`` counts the diagonal twice and breaks ties by node order
(matrix.py:80-104), ``lock()`` makes writes fail (matrix.py:308-309).
"""

import logging
import os

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


# ---------------------------------------------------------------------------------------
# matrix_de_novo
# ---------------------------------------------------------------------------------------
def _outside_in_index_iterator(num_indices):
    """Indices from both ends toward the middle: 5 -> 0, 4, 1, 3, 2 (matrix.py:409-423)."""
    lo, hi = 0, num_indices - 1
    while lo < hi:
        yield lo
        yield hi
        lo, hi = lo + 1, hi - 1
    if lo == hi:
        yield lo


def calculate_adjacency(source, target, func, distance=True):
    return source.name, target.name, func(source, target, as_distance=distance)


_CONTEXTS = {}


def default_device():
    """PHAMCLUST_DEVICE, else this rank's LOCAL_RANK (one process per GPU under torch.distributed.run), else 0."""
    if "PHAMCLUST_DEVICE" not in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        from phamclust_amd import distributed
        return distributed.local_device()
    return int(os.environ.get("PHAMCLUST_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def get_context(device_id=None):
    """One cached HIP context per device for the life of the process."""
    from phamclust_amd import hip
    device_id = default_device() if device_id is None else device_id
    if device_id not in _CONTEXTS:
        _CONTEXTS[device_id] = hip.Context(device_id)
    return _CONTEXTS[device_id]


def in_process_devices():
    """Device ordinals of an in-process multi-GPU fill, or None: ``PHAMCLUST_GPUS=N`` (what ``phamclust --gpus N`` sets when it
    keeps the job in this process) -> devices 0..N-1; ``PHAMCLUST_GPU_IDS=0,0,1`` names them (an id may repeat: rehearsal on a box
    with fewer GPUs).  Ignored under a launcher (WORLD_SIZE > 1: one process per GPU is then the job's shape)."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return None
    ids = os.environ.get("PHAMCLUST_GPU_IDS")
    if ids:
        return [int(x) for x in ids.split(",")]
    n = int(os.environ.get("PHAMCLUST_GPUS", "1"))
    return list(range(n)) if n > 1 else None


def get_multi_context(device_ids):
    from phamclust_amd import hip
    key = ("multi",) + tuple(device_ids)
    if key not in _CONTEXTS:
        try:
            _CONTEXTS[key] = hip.MultiContext(device_ids)
        except hip.HipLibraryError as exc:
            raise hip.HipLibraryError(f"{exc} -- asked for devices {list(device_ids)} (--gpus / PHAMCLUST_GPUS / PHAMCLUST_GPU_IDS): "
                                      f"ask for the GPUs this node has, or name them with PHAMCLUST_GPU_IDS") from None
    return _CONTEXTS[key]


def _metric_name(func):
    from phamclust_amd import metrics
    return metrics.ACCELERATED.get(func)


NEAREST_MAX_K = 64      # PC_NEAREST_MAX_K of the C-ABI: the k a nearest-neighbours fill takes at most
BETWEEN_MAX_GROUPS = 2048   # PC_BETWEEN_MAX_GROUPS of the C-ABI: the groups a between-groups fill takes at most
LAST_FILL = {}          # what the last accelerated matrix_de_novo did: the pipeline's log line reads it


def _packed_of(genomes):
    """The packed form of ``genomes``: the loader's own arrays when the list is exactly what the C loader produced
    (pack.load_tsv_genomes: untouched lazy genomes, all of them, in order), else a fresh pack of the objects."""
    from phamclust_amd.pack import pack_genomes, packed_behind
    return packed_behind(genomes) or pack_genomes(genomes)


def matrix_de_novo(genomes, func, cpus, as_distance=True):
    """Fill an N x N ``SymMatrix`` with ``func`` over every genome pair (matrix.py:432-497).

    The six METRICS run on the GPU.  Where the reference spreads the pairs over ``cpus`` worker processes
    (matrix.py:471-472), this spreads them over the GPUs of the job it runs in: under
    ``python -m torch.distributed.run --nproc-per-node N`` (one process per GPU; ``phamclust --gpus N`` starts that
    for you) every rank calls this with the same genomes, fills its static shard of the pair list, and ONE gather
    brings the shards to rank 0.  Rank 0 returns the matrix; every other rank returns ``None``.  Without a launcher,
    ``PHAMCLUST_GPUS=N`` (set by ``phamclust --gpus N``) spreads the same shards over N GPUs from THIS process (``pc_multi_*``:
    a host thread per device inside the library, device-to-device copies for the exchange).  For those six, ``cpus`` is
    accepted for signature compatibility only; any OTHER callable is filled the reference's way -- per pair, in its batch
    order, over ``cpus`` joblib workers (in this process when ``cpus`` is 1).
    """
    if len(genomes) == 0:
        raise ValueError("need at least 1 genome to construct matrix de novo")
    names = [g.name for g in genomes]
    metric = _metric_name(func)
    if metric is not None:
        import time
        from phamclust_amd import distributed
        rank, world = distributed.ensure_process_group()          # before the first GPU call of this process
        t0 = time.perf_counter()
        packed = _packed_of(genomes)
        t1 = time.perf_counter()
        devices = in_process_devices()
        ctx = get_multi_context(devices) if devices else get_context()
        # gcs / jc / pocp / af never read a residue (metrics.py:26-157): their upload skips the residue stage
        ctx.upload(packed, residues=metric in ("aai", "peq"))
        t2 = time.perf_counter()
        if world > 1:
            condensed, stats = distributed.fill_condensed(ctx, metric, as_distance)
        else:                                              # one process: one GPU, or several through pc_multi_* (no launcher, no process group)
            condensed, stats = ctx.fill(metric, as_distance=as_distance, want_stats=True, borrow=True)
        t3 = time.perf_counter()
        LAST_FILL.clear()
        LAST_FILL.update(stats, metric=metric, n_genomes=len(genomes), genome_pairs=packed.n_pairs, n_gpus=len(devices) if devices else world, rank=rank,
                         pack_s=t1 - t0, upload_s=t2 - t1, fill_s=t3 - t2)
        logging.debug(f"{len(genomes)} genomes -> {packed.n_pairs} edges on {world} device(s): pack {t1 - t0:.3f} s, "
                      f"upload {t2 - t1:.3f} s, fill+gather+D2H {t3 - t2:.3f} s (kernels {stats['ms_total']:.3f} ms on this rank)")
        if condensed is None:
            return None
        return SymMatrix.from_condensed(names, condensed, is_distance=as_distance)

    # any other callable: the reference's per-pair semantics, its batch order, its worker pool (matrix.py:460-493)
    n = len(genomes)
    n_pairs = n * (n - 1) // 2 + n
    if n_pairs < cpus:                                  # (matrix.py:460-462)
        logging.info(f"small dataset - reducing # CPUs to {n_pairs}")
        cpus = n_pairs
    matrix = SymMatrix(nodes=names, is_distance=as_distance)
    for genome in genomes:
        matrix.set_weight(genome.name, genome.name, 1.0 - as_distance)
    order = list(_outside_in_index_iterator(n))
    if cpus is None or cpus <= 1:
        for i in order:
            source = genomes[i]
            for target in genomes[i + 1:]:
                s, t, w = calculate_adjacency(source, target, func, as_distance)
                matrix.set_weight(s, t, w)
        return matrix
    # Batches of `stride` source rows in outside-in order hold about 10,000 pairs per worker (matrix.py:474-478); inside a batch
    # one task is one SOURCE ROW cut into pieces of at most 2,500 targets -- the reference pickles both genomes of every pair
    # (matrix.py:484-488), this sends a source once per piece -- and results come back in whatever order the workers finish.
    import joblib
    stride = max(1, int(n // (n_pairs / (10000 * cpus))))
    runner = joblib.Parallel(n_jobs=cpus, return_as="generator_unordered", max_nbytes=None)
    for b0 in range(0, n, stride):
        rows = order[b0:b0 + stride]
        pieces = [(genomes[i], genomes[j0:min(j0 + 2500, n)]) for i in rows for j0 in range(i + 1, n, 2500)]
        for edges in runner(joblib.delayed(_row_adjacency)(source, targets, func, as_distance) for source, targets in pieces):
            for s, t, w in edges:
                matrix.set_weight(s, t, w)
        logging.debug(f"finished {', '.join(genomes[i].name for i in rows)}")
    del runner
    return matrix


def _row_adjacency(source, targets, func, distance):
    """One worker task of the generic path: ``source`` against a run of targets."""
    return [calculate_adjacency(source, target, func, distance) for target in targets]


def _pairs_adjacency(pairs, func, distance):
    """One worker task of matrix_extend's generic path: a run of (source, target) pairs."""
    return [calculate_adjacency(source, target, func, distance) for source, target in pairs]


def _square_matrix(nodes, data, is_distance):
    """A SymMatrix over ``nodes`` that takes ``data`` (N x N, already rounded, diagonal set) as its storage."""
    m = SymMatrix.__new__(SymMatrix)
    m._nodes = list(nodes)
    m._slot = {name: k for k, name in enumerate(m._nodes)}
    m._data = data
    m._is_distance = is_distance
    m._locked = False
    return m


def matrix_extend(matrix, genomes, func, cpus, verify=4):
    """New genomes against a filled matrix: the ``SymMatrix`` over all of ``genomes`` (in that order -- the fill order, which
    is name-sorted in the pipeline) that ``matrix_de_novo(genomes, func, cpus, matrix.is_distance)`` would return, computing
    only the pairs ``matrix`` lacks.  ``matrix`` holds a subset of the genomes' names; its block is copied, the rows of the
    genomes it lacks come from ONE rows fill (``Context.fill_rows``: k new genomes cost k N pairs, not N^2 / 2).  The reference
    has the container half of this (``SymMatrix.append_node``, matrix.py:169-213) and nothing that produces the values.

    ``verify`` old genomes -- spread evenly over the old ones in list order, at most all of them -- are refilled with the new
    rows, and every refilled value must EQUAL the stored one: the guard against a stale file, another metric, a changed genome
    or another genome order (pair orientation follows the order, and aai is not symmetric).  A mismatch raises ``ValueError``
    naming the first differing pair; ``verify=0`` switches the guard off.

    Nothing new: the matrix re-laid in ``genomes`` order.  Every genome new: ``matrix_de_novo``.  An unset (NaN) old cell:
    ``ValueError``.  A node of ``matrix`` that is no genome: ``KeyError`` (``extract_submatrix`` the shared nodes first).  A
    callable outside ``METRICS`` is run per new pair on the host (over ``cpus`` joblib workers), the reference's way.  One GPU:
    with ``PHAMCLUST_GPUS`` / ``PHAMCLUST_GPU_IDS`` the first listed device; under a launcher (``WORLD_SIZE`` > 1) it raises.
    """
    if len(genomes) == 0:
        raise ValueError("need at least 1 genome to extend a matrix")
    names = [g.name for g in genomes]
    index = {name: k for k, name in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("genome names must be distinct")
    stranger = next((node for node in matrix.nodes if node not in index), None)
    if stranger is not None:
        raise KeyError(f"node '{stranger}' of the matrix is not among the genomes: extract_submatrix() the nodes they share first")
    as_distance = matrix.is_distance
    n = len(names)
    old_idx = [k for k, name in enumerate(names) if name in matrix]
    new_idx = [k for k, name in enumerate(names) if name not in matrix]
    if not old_idx:
        return matrix_de_novo(genomes, func, cpus, as_distance=as_distance)
    slots = np.fromiter((matrix._slot[names[k]] for k in old_idx), dtype=np.int64, count=len(old_idx))
    block = matrix._data[np.ix_(slots, slots)]
    if np.isnan(block).any():
        i, j = (int(x) for x in np.argwhere(np.isnan(block))[0])
        raise ValueError(f"the matrix has an unset cell ({names[old_idx[i]]}, {names[old_idx[j]]}): only a filled matrix can be extended")
    if not new_idx:
        return _square_matrix(names, block.copy(), as_distance)
    old_at = np.asarray(old_idx, dtype=np.int64)
    full = np.full((n, n), np.nan, dtype=np.float64)
    full[np.ix_(old_at, old_at)] = block
    metric = _metric_name(func)
    if metric is not None:
        import time
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise RuntimeError("matrix_extend: the rows fill is a one-GPU call; run it in one process, not under a launcher (WORLD_SIZE > 1)")
        devices = in_process_devices()
        if devices:
            logging.debug(f"matrix_extend: the rows fill is a one-GPU call: using device {devices[0]} of {devices}")
        t0 = time.perf_counter()
        packed = _packed_of(genomes)
        t1 = time.perf_counter()
        ctx = get_context(devices[0] if devices else None)
        ctx.upload(packed, residues=metric in ("aai", "peq"))
        t2 = time.perf_counter()
        n_verify = max(0, min(int(verify), len(old_idx)))
        checked = sorted({old_idx[(i * len(old_idx)) // n_verify] for i in range(n_verify)})
        rows = sorted(set(new_idx) | set(checked))
        values, stats = ctx.fill_rows(metric, rows, as_distance=as_distance, want_stats=True)
        t3 = time.perf_counter()
        row_at = {q: k for k, q in enumerate(rows)}
        for q in checked:
            stored, refilled = full[q, old_at], values[row_at[q], old_at]
            if not np.array_equal(stored, refilled):
                g = int(old_at[np.flatnonzero(stored != refilled)[0]])
                raise ValueError(f"pair ({names[min(q, g)]}, {names[max(q, g)]}): the matrix holds {full[q, g]!r}, the {metric} fill gives "
                                 f"{values[row_at[q], g]!r}: the matrix was not filled with this metric from these genomes in this order")
        for q in new_idx:
            full[q, :] = values[row_at[q]]
            full[:, q] = values[row_at[q]]
        LAST_FILL.clear()
        LAST_FILL.update(stats, metric=metric, n_genomes=n, genome_pairs=int(stats["n_pairs"]), rows=len(rows), n_gpus=1, rank=0,
                         pack_s=t1 - t0, upload_s=t2 - t1, fill_s=t3 - t2)
        logging.debug(f"{len(new_idx)} new of {n} genomes -> {len(rows)} rows, {stats['n_pairs']} edges on one device: pack {t1 - t0:.3f} s, "
                      f"upload {t2 - t1:.3f} s, fill+D2H {t3 - t2:.3f} s (kernels {stats['ms_total']:.3f} ms)")
        return _square_matrix(names, full, as_distance)

    # any other callable: the reference's per-pair semantics over the new pairs only, source = the earlier genome of the list
    result = _square_matrix(names, full, as_distance)
    is_new = set(new_idx)
    pairs = [(genomes[min(q, g)], genomes[max(q, g)]) for q in new_idx for g in range(n) if g != q and not (g in is_new and g < q)]
    for q in new_idx:
        result.set_weight(names[q], names[q], 1.0 - as_distance)
    if cpus is None or cpus <= 1 or len(pairs) < 2 * cpus:
        batches = [_pairs_adjacency(pairs, func, as_distance)]
    else:
        import joblib
        step = max(1, min(2500, (len(pairs) + cpus - 1) // cpus))
        runner = joblib.Parallel(n_jobs=cpus, return_as="generator_unordered", max_nbytes=None)
        batches = runner(joblib.delayed(_pairs_adjacency)(pairs[i:i + step], func, as_distance) for i in range(0, len(pairs), step))
    for edges in batches:
        for s, t, w in edges:
            result.set_weight(s, t, w)
    return result


# ---------------------------------------------------------------------------------------
# TSV I/O: adjacency, squareform, lower triangle (matrix.py:500-670); "%.6f" everywhere
# ---------------------------------------------------------------------------------------
def read_adjacency(filepath):
    with open(filepath, "r") as handle:
        for line in handle:
            fields = line.rstrip().split("\t")
            yield fields[0], fields[1], float(fields[2])


def _diagonal_kind(diagonal, count):
    if len(diagonal) > 1:
        raise ValueError("values on matrix diagonal should be identical")
    total = sum(diagonal)
    if total == 0.0:
        return True
    if total == count:
        return False
    raise ValueError("values on matrix diagonal can only be 0.0 or 1.0")


def matrix_from_adjacency(filepath):
    names, diagonal = dict(), set()
    for source, target, weight in read_adjacency(filepath):
        if source == target:
            diagonal.add(weight)
        if target in names:
            break
        names[target] = None
    matrix = SymMatrix(list(names), is_distance=_diagonal_kind(diagonal, 1.0))
    for source, target, weight in read_adjacency(filepath):
        matrix.set_weight(source, target, weight)
    return matrix


_TEXT_LIB = None


def _text_lib():
    """csrc/libpc_pack.so's row formatter / parser ("%.6f", byte for byte), or None when it is not built: the text
    I/O then runs in Python (same bytes, ~100x slower at N = 10,000)."""
    global _TEXT_LIB
    if _TEXT_LIB is None:
        import ctypes
        import os
        from phamclust_amd.build import native_path
        path = native_path("libpc_pack.so")
        try:
            lib = ctypes.CDLL(path)
            lib.pcp_format_row.restype = ctypes.c_int64
            lib.pcp_format_row.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64]
            lib.pcp_format_adjacency.restype = ctypes.c_int64
            lib.pcp_format_adjacency.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
            lib.pcp_format_edges.restype = ctypes.c_int64
            lib.pcp_format_edges.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
            lib.pcp_parse_row.restype = ctypes.c_int64
            lib.pcp_parse_row.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
            _TEXT_LIB = lib
        except (OSError, AttributeError):
            _TEXT_LIB = False
    return _TEXT_LIB or None


def matrix_to_adjacency(matrix, filepath, skip_zero=False):
    lib = _text_lib() if isinstance(matrix, SymMatrix) else None
    data = matrix._ordered() if lib else None
    if lib is None or np.isnan(data).any():                 # unset cells: the reference's formatting error surfaces below
        with open(filepath, "w") as handle:
            for source, target, weight in matrix:
                if skip_zero and not weight:
                    continue
                handle.write(f"{source}\t{target}\t{weight:.6f}\n")
        return filepath
    import ctypes
    names = [name.encode() for name in matrix.nodes]
    blob = b"".join(names)
    offsets = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in names], out=offsets[1:])
    n = len(names)
    width = (max((len(x) for x in names), default=0)) * 2 + 32
    cap = n * width + 1024
    buf = ctypes.create_string_buffer(cap)
    data = np.ascontiguousarray(data, dtype=np.float64)
    with open(filepath, "wb") as handle:
        for i, source in enumerate(names):
            size = lib.pcp_format_adjacency(source, len(source), blob, offsets.ctypes.data, data[i].ctypes.data, i, n,
                                            1 if skip_zero else 0, buf, cap)
            if size < 0:
                raise ValueError(f"{filepath}: a row of '{source.decode()}' does not fit its buffer (weights outside [0, 1]?)")
            handle.write(buf.raw[:size] if size < 65536 else memoryview(buf)[:size])
    return filepath


# ---------------------------------------------------------------------------------------
# Sparse delivery: the pairs within a threshold, without the dense matrix
# ---------------------------------------------------------------------------------------
def _grown_positions(stored_nodes, nodes, rows, caller):
    """What the host statements of the ``*_extend`` calls share: ``old_at[k]`` = the position in ``nodes`` of stored node k (int64,
    strictly increasing, else ValueError; KeyError for a stored node ``nodes`` lacks) and ``rows`` as an ascending int64 array that
    must name exactly the positions of the nodes that are not stored."""
    nodes = list(nodes)
    index = {name: k for k, name in enumerate(nodes)}
    if len(index) != len(nodes):
        raise ValueError(f"{caller}: node names must be distinct")
    stranger = next((node for node in stored_nodes if node not in index), None)
    if stranger is not None:
        raise KeyError(f"{caller}: stored node '{stranger}' is not among the nodes")
    old_at = np.fromiter((index[node] for node in stored_nodes), dtype=np.int64, count=len(stored_nodes))
    if old_at.shape[0] > 1 and not (np.diff(old_at) > 0).all():
        k = int(np.flatnonzero(np.diff(old_at) <= 0)[0])
        raise ValueError(f"{caller}: stored nodes '{stored_nodes[k]}' and '{stored_nodes[k + 1]}' come in another order in the grown collection: "
                         "orientation and tie order follow the order, so a result can only be grown in its own order")
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    is_old = np.zeros(len(nodes), dtype=bool)
    is_old[old_at] = True
    if not np.array_equal(rows, np.flatnonzero(~is_old)):
        raise ValueError(f"{caller}: rows must be the ascending positions of exactly the nodes that are not stored")
    return old_at, rows


def _live_row_pairs(n, rows, values):
    """The pairs of a rows array, each once: ``values[i, g]`` is the pair {rows[i], g}; the diagonal is none, and a pair of two
    rows is taken in the row of the smaller one (the rule of the library's rows passes).  Returns (source, target, weight) with
    source < target, row-major."""
    values = np.asarray(values, dtype=np.float64).reshape(len(rows), n)
    if len(rows) == 0:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64)
    is_row = np.zeros(n, dtype=bool)
    is_row[rows] = True
    q = np.repeat(rows, n).reshape(len(rows), n)
    g = np.tile(np.arange(n, dtype=np.int64), (len(rows), 1))
    live = (g != q) & ~(is_row[g] & (g < q))
    q, g = q[live], g[live]
    return np.minimum(q, g), np.maximum(q, g), values[live]


def _positions_without(nodes, names, caller):
    """(positions kept, ascending; new position of every old one or -1) of ``nodes`` without ``names`` (KeyError for a stranger)."""
    index = {name: k for k, name in enumerate(nodes)}
    drop = set()
    for name in names:
        if name not in index:
            raise KeyError(f"{caller}: '{name}' is not among the nodes")
        drop.add(index[name])
    keep_at = np.asarray([k for k in range(len(nodes)) if k not in drop], dtype=np.int64)
    new_at = np.full(len(nodes), -1, dtype=np.int64)
    new_at[keep_at] = np.arange(keep_at.shape[0])
    return keep_at, new_at


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
        keep = np.flatnonzero((w <= threshold) if matrix.is_distance else (w >= threshold))
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

    def components(self, threshold=None, strict=True):
        """Connected components of the graph over ``nodes`` whose edges are this list's pairs within ``threshold`` -- ``weight <
        threshold`` on distances, ``> threshold`` on similarities; ``<=`` / ``>=`` with ``strict=False``; ``None``: every pair
        of the list -- as int32 labels, ``labels[g]`` = the smallest index of g's component.  On distances with ``strict`` these are
        the single-linkage clusters at ``eps = threshold`` (scikit-learn merges below its ``distance_threshold``, never at it).  Host
        arithmetic (``scipy.sparse.csgraph``): the statement ``Context.fill_components`` is held to."""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        n = len(self.nodes)
        if threshold is None:
            keep = np.ones(len(self), dtype=bool)
        elif self.is_distance:
            keep = self.weight < threshold if strict else self.weight <= threshold
        else:
            keep = self.weight > threshold if strict else self.weight >= threshold
        src, tgt = self.source[keep], self.target[keep]
        graph = coo_matrix((np.ones(src.shape[0], dtype=np.int8), (src, tgt)), shape=(n, n))
        _, comp = connected_components(graph, directed=False)
        smallest = np.full(int(comp.max()) + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(smallest, comp, np.arange(n))
        return smallest[comp].astype(np.int32)

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
        keep = (w <= self.threshold) if self.is_distance else (w >= self.threshold)
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


def _slab_fill_context():
    """(context, devices used) of an edge-list, components, nearest-neighbours or tree fill: the ``MultiContext`` over the devices
    ``in_process_devices()`` names when there are several -- the four fills spread over them, a stretch of targets per device --
    else the one-GPU context (of the one device named, or the default device)."""
    devices = in_process_devices()
    if devices and len(devices) > 1:
        return get_multi_context(devices), len(devices)
    return get_context(devices[0] if devices else None), 1


def edges_de_novo(genomes, func, threshold, as_distance=True, slab_bytes=0):
    """The edges of ``matrix_de_novo(genomes, func, cpus, as_distance)`` within ``threshold`` as a :class:`SparseEdges`, filled
    on the GPU by ``Context.fill_edges``: the dense matrix is never delivered, and beyond ``slab_bytes`` of HBM (0: automatic)
    never held.  ``func`` must be one of the six ``METRICS`` callables: there is no CPU route for this call (a generic callable
    has ``matrix_de_novo`` and ``SparseEdges.from_dense``).  With ``PHAMCLUST_GPUS`` / ``PHAMCLUST_GPU_IDS`` naming more than one
    device the fill is spread over them from this process (``MultiContext.fill_edges``: a contiguous stretch of targets per device,
    the same edges); under a launcher (``WORLD_SIZE`` > 1) it raises."""
    names, (src, tgt, val) = _de_novo_route(genomes, func, "edges_de_novo",
        lambda ctx, metric: ctx.fill_edges(metric, threshold, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: (
            f"{len(genomes)} genomes -> {stats['n_edges']} of {record['genome_pairs']} edges in {stats['n_slabs']} slab(s) on {record['n_gpus']} "
            f"device(s): fill+compact+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)"),
        advice="for another callable: SparseEdges.from_dense(matrix_de_novo(...), threshold)")
    return SparseEdges(names, src, tgt, val, is_distance=as_distance, threshold=threshold)


class Components:
    """A partition of ``nodes`` into connected components: ``labels[g]`` is the smallest index of g's component (what
    ``Context.fill_components`` and ``SparseEdges.components`` deliver)."""

    def __init__(self, nodes, labels):
        self.nodes = list(nodes)
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        if self.labels.shape != (len(self.nodes),):
            raise ValueError("labels must hold one entry per node")
        at = np.arange(len(self.nodes))
        if len(self.nodes) and not ((self.labels >= 0).all() and (self.labels <= at).all() and (self.labels[self.labels] == self.labels).all()):
            raise ValueError("labels[g] must be the smallest index of g's component")

    @property
    def n_components(self):
        return int((self.labels == np.arange(len(self.nodes))).sum())

    def __len__(self):
        return self.n_components

    def group_indices(self):
        """The components as index arrays in the order ``hierarchical_clustering`` returns its parts: largest first, equal sizes
        in order of their smallest member (``sorted(parts, reverse=True)`` over first-appearance order: Python's reverse sort is
        stable), members ascending."""
        order = np.argsort(self.labels, kind="stable")                         # grouped by label = by smallest member, members ascending
        roots, starts = np.unique(self.labels[order], return_index=True)
        groups = np.split(order, starts[1:]) if len(roots) else []
        return sorted(groups, key=len, reverse=True)

    def groups(self):
        """The same as lists of node names."""
        return [[self.nodes[i] for i in group.tolist()] for group in self.group_indices()]

    def extended(self, nodes, rows, values, threshold, is_distance=True, strict=True):
        """This partition grown to ``nodes``: the host statement of ``components_extend`` (arguments as ``SparseEdges.extended``;
        ``threshold``, ``is_distance`` and ``strict`` say which new pairs are edges, as ``SparseEdges.components`` does).  The stored
        labels, re-indexed, are the forest the passing new pairs are united into; labels stay the smallest member's index."""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        old_at, rows = _grown_positions(self.nodes, nodes, rows, "Components.extended")
        n = len(nodes)
        src, tgt, w = _live_row_pairs(n, rows, values)
        if is_distance:
            keep = w < threshold if strict else w <= threshold
        else:
            keep = w > threshold if strict else w >= threshold
        src = np.concatenate([old_at[self.labels], src[keep]])
        tgt = np.concatenate([old_at, tgt[keep]])
        graph = coo_matrix((np.ones(src.shape[0], dtype=np.int8), (src, tgt)), shape=(n, n))
        _, comp = connected_components(graph, directed=False)
        smallest = np.full(int(comp.max()) + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(smallest, comp, np.arange(n))
        return Components(nodes, smallest[comp].astype(np.int32))

    def without(self, names):
        """This partition restricted to the genomes that remain: every group loses the members named, labels stay the smallest
        member's index.  Each group that remains is a union of whole components of the smaller collection, and the components of
        the smaller collection itself wherever the genomes removed were no articulation points: a component held together only by
        a removed genome stays one group here (the labels do not say which pairs were edges).  ``SparseEdges.without(names)
        .components(...)`` is exact; so is a components fill of the remaining genomes."""
        keep_at, _ = _positions_without(self.nodes, names, "Components.without")
        labels = self.labels[keep_at]
        _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)       # first member kept of every group = its smallest
        return Components([self.nodes[k] for k in keep_at.tolist()], first[inverse].astype(np.int32))


def components_de_novo(genomes, func, threshold, as_distance=True, strict=True, slab_bytes=0):
    """The connected components of the graph {pairs of ``matrix_de_novo(genomes, func, cpus, as_distance)`` within ``threshold``}
    (``<`` on distances, ``>`` on similarities; ``<=`` / ``>=`` with ``strict=False``) as a :class:`Components`, by
    ``Context.fill_components``: neither the dense matrix nor an edge list leaves the GPU, only the N labels.  On distances with
    ``strict`` the groups are ``hierarchical_clustering(matrix, "single", eps=threshold)``'s.  ``func`` must be one of the six
    ``METRICS`` callables (no CPU route: ``SparseEdges.from_dense(matrix_de_novo(...), 2.0).components(threshold)`` serves another
    callable).  Several devices as ``edges_de_novo`` (``MultiContext.fill_components``: the same labels); under a launcher
    (``WORLD_SIZE`` > 1) it raises."""
    names, (labels,) = _de_novo_route(genomes, func, "components_de_novo",
        lambda ctx, metric: ctx.fill_components(metric, threshold, as_distance=as_distance, strict=strict, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: (
            f"{len(genomes)} genomes -> {stats['n_components']} components from {stats['n_edges']} of {record['genome_pairs']} pairs in "
            f"{stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): fill+union+labels {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)"),
        advice="for another callable: SparseEdges.from_dense(matrix_de_novo(...), 2.0).components(threshold)")
    return Components(names, labels)


def upload_for_fills(genomes, func, caller, several=False, advice="the dense route, matrix_de_novo, serves another callable"):
    """What the one-GPU routes without a dense matrix share ahead of their fills: the refusals (no genome, a callable outside the
    six ``METRICS``, a launcher), then ONE pack and ONE upload.  Returns ``(context, metric name, genome names, record)`` -- the
    record holds ``pack_s``, ``upload_s``, ``n_gpus`` and the collection's ``genome_pairs`` for ``LAST_FILL`` -- and the caller runs as
    many fills as it needs.  ``several``: the caller's fill also runs over several devices (``edges_de_novo``, ``components_de_novo``,
    ``neighbors_de_novo``, ``tree_de_novo``), so the context is ``_slab_fill_context()``'s; the groups and rows routes leave it off and stay on one GPU.
    ``advice``: what the refusal of a generic callable tells its reader to use instead.  The caller runs as many fills
    on the context as it needs (``submatrices_de_novo``: a groups fill; ``hierarchical_clustering_de_novo``: a components fill, then
    a groups fill; ``phamclust --no-matrix``: two and three of them)."""
    if len(genomes) == 0:
        raise ValueError(f"{caller}: need at least 1 genome")
    metric = _metric_name(func)
    if metric is None:
        raise ValueError(f"{caller}: func must be one of the six METRICS callables -- the components and groups fills run on the GPU only and "
                         f"have no CPU route ({advice})")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError(f"{caller}: the components and groups fills are one-GPU calls; run it in one process, not under a launcher (WORLD_SIZE > 1)")
    import time
    devices = in_process_devices()
    if devices and not (several and len(devices) > 1):
        logging.debug(f"{caller}: one-GPU calls: using device {devices[0]} of {devices}")
    t0 = time.perf_counter()
    packed = _packed_of(genomes)
    t1 = time.perf_counter()
    ctx, n_gpus = _slab_fill_context() if several else (get_context(devices[0] if devices else None), 1)
    ctx.upload(packed, residues=metric in ("aai", "peq"))
    t2 = time.perf_counter()
    logging.debug(f"{caller}: {len(genomes)} genomes: pack {t1 - t0:.3f} s, upload {t2 - t1:.3f} s")
    return ctx, metric, [g.name for g in genomes], dict(pack_s=t1 - t0, upload_s=t2 - t1, genome_pairs=packed.n_pairs, n_gpus=n_gpus)


def _fill_done(stats, metric, names, record, t0, log, **own):
    """After the one fill of a ``*_de_novo`` / ``*_extend`` route, begun at ``t0``: ``LAST_FILL`` -- the fill's stats, the collection, the
    upload's record and the route's ``own`` entries -- and the route's log line, ``log(stats, record, fill_s)``."""
    import time
    fill_s = time.perf_counter() - t0
    LAST_FILL.clear()
    LAST_FILL.update(stats, metric=metric, n_genomes=len(names), rank=0, pack_s=record["pack_s"], upload_s=record["upload_s"], fill_s=fill_s, **own)
    logging.debug(log(stats, record, fill_s))


def _de_novo_route(genomes, func, caller, fill, log, advice="the dense route, matrix_de_novo, serves another callable"):
    """The frame the four ``*_de_novo`` routes share: ``upload_for_fills`` over the devices at hand (``advice``: its refusal's), the clock,
    ``fill(ctx, metric)`` -> ``(*arrays, stats)``, ``LAST_FILL`` and the log line (``_fill_done``).  Returns ``(names, arrays)``."""
    ctx, metric, names, record = upload_for_fills(genomes, func, caller, several=True, advice=advice)
    import time
    t0 = time.perf_counter()
    *arrays, stats = fill(ctx, metric)
    _fill_done(stats, metric, names, record, t0, log, genome_pairs=record["genome_pairs"], n_gpus=record["n_gpus"])
    return names, arrays


def _group_indices(names, index, groups):
    """``groups`` -- each a sequence of genome names or of indices into the genome list -- as ascending index lists.  KeyError
    for an unknown name, IndexError for an index outside the list, ValueError for a genome twice in one group."""
    out = []
    for k, group in enumerate(groups):
        idx = []
        for member in group:
            if isinstance(member, (int, np.integer)) and not isinstance(member, bool):
                if not 0 <= int(member) < len(names):
                    raise IndexError(f"group {k}: genome index {int(member)} is outside 0..{len(names) - 1}")
                idx.append(int(member))
            elif member in index:
                idx.append(index[member])
            else:
                raise KeyError(f"group {k}: '{member}' is not among the genomes")
        if len(set(idx)) != len(idx):
            twice = next(names[i] for i in idx if idx.count(i) > 1)
            raise ValueError(f"group {k}: genome '{twice}' is listed twice")
        out.append(sorted(idx))
    return out


def submatrices_de_novo(genomes, func, groups, as_distance=True):
    """``[matrix_de_novo(genomes, func, cpus, as_distance).extract_submatrix(names of group) for group in groups]`` without the
    N x N matrix: one ``SymMatrix`` per group, filled by ONE groups fill (``Context.fill_groups``) -- one pack and one upload
    whatever the number of groups, sum of n_c^2 cells instead of N^2, and a sequence pair that occurs in several groups aligned
    once.  A group is a sequence of genome names or of indices into ``genomes``; groups may share genomes.  Each matrix's nodes are
    the group's genomes in genome-list order, so every pair keeps the whole fill's orientation and its value bit for bit (aai
    included); a group of one gives a one-node matrix with the diagonal preset (matrix.py:467-468), an empty group an empty matrix.
    ``func`` must be one of the six ``METRICS`` callables (no CPU route).  One GPU, as ``edges_de_novo``: under a launcher
    (``WORLD_SIZE`` > 1) it raises.  Every refusal comes before the first GPU call."""
    names = [g.name for g in genomes]
    index = {name: k for k, name in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("genome names must be distinct")
    members = _group_indices(names, index, groups)
    ctx, metric, names, record = upload_for_fills(genomes, func, "submatrices_de_novo")
    import time
    t0 = time.perf_counter()
    parts, stats = ctx.fill_groups(metric, members, as_distance=as_distance, want_stats=True)
    fill_s = time.perf_counter() - t0
    LAST_FILL.clear()
    LAST_FILL.update(stats, metric=metric, n_genomes=len(genomes), genome_pairs=int(stats["n_pairs"]), groups=len(members), n_gpus=1, rank=0,
                     pack_s=record["pack_s"], upload_s=record["upload_s"], fill_s=fill_s)
    logging.debug(f"{len(genomes)} genomes, {len(members)} groups -> {stats['n_pairs']} of {record['genome_pairs']} edges on one device: "
                  f"fill+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)")
    out = []
    for idx, condensed in zip(members, parts):
        nodes = [names[i] for i in idx]
        if len(nodes) < 2:
            one = SymMatrix(nodes=nodes, is_distance=as_distance)
            for node in nodes:
                one.set_weight(node, node, 1.0 - as_distance)
            out.append(one)
        else:
            out.append(SymMatrix.from_condensed(nodes, condensed, is_distance=as_distance))
    return out


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


def neighbors_de_novo(genomes, func, k, as_distance=True, slab_bytes=0):
    """Each genome's ``k`` nearest neighbours in ``matrix_de_novo(genomes, func, cpus, as_distance)`` as a
    :class:`NearestNeighbors`, filled on the GPU by ``Context.fill_nearest``: the dense matrix is never delivered, and beyond
    ``slab_bytes`` of HBM (0: automatic) never held; N * k entries cross PCIe.  ``func`` must be one of the six ``METRICS``
    callables (no CPU route: ``NearestNeighbors.from_dense(matrix_de_novo(...), k)`` serves another callable).  Several devices as
    ``edges_de_novo`` (``MultiContext.fill_nearest``: the same lists); under a launcher (``WORLD_SIZE`` > 1) it raises.  Every
    refusal comes before the first GPU call."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= NEAREST_MAX_K:
        raise ValueError(f"neighbors_de_novo: k must be an integer in 1..{NEAREST_MAX_K}, not {k!r}")
    names, (nbr, val) = _de_novo_route(genomes, func, "neighbors_de_novo",
        lambda ctx, metric: ctx.fill_nearest(metric, int(k), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: f"{len(genomes)} genomes -> {stats['k']} nearest neighbours each from {record['genome_pairs']} pairs in "
                                      f"{stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): fill+select+D2H {fill_s:.3f} s (kernels "
                                      f"{stats['ms_total']:.3f} ms, selection {stats.get('ms_select', 0.0):.3f} ms)")
    return NearestNeighbors(names, nbr, val, is_distance=as_distance)


def _kruskal(n, s, t, w, is_distance):
    """Kruskal's algorithm over the pairs (s[e], t[e]) of weight w[e] in the tree's total order -- ``np.lexsort`` over (source, target,
    weight): the weight first, better first -- with a union-find: the indices of the accepted pairs, in that order."""
    order = np.lexsort((s, t, w if is_distance else -w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    kept = []
    for e, a, b in zip(order.tolist(), s[order].tolist(), t[order].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            kept.append(e)
            if len(kept) == n - 1:
                break
    return np.asarray(kept, dtype=np.int64)


class SingleLinkageTree:
    """The single-linkage dendrogram of a matrix as the ``N - 1`` edges of its minimum spanning tree, in merge order: ``source[i] <
    target[i]`` (indices into ``nodes``) joined at ``weight[i]``.  ONE total order on the pairs decides everything: the better weight
    first -- the smaller on distances, the larger on similarities, a plain float compare -- then the smaller target, then the
    smaller source; the tree is the one Kruskal's algorithm accepts when it takes the pairs in that order, so it is unique, ties
    included.  The reference derives the same dendrogram from its dense matrix (``scipy.cluster.hierarchy.linkage(..., 'single')``
    in ``_get_tree_order``, matrix.py:673-686; scikit-learn's single linkage in clustering.py:4-51); ``tree_de_novo`` fills it on the
    GPU without the dense matrix, ``from_dense`` states it on the host.  Clusters at any threshold (``cut``), for any cluster count
    (``cut_n``), scipy's ``Z`` (``linkage``) and the leaf order (``leaves``) follow from the edges alone."""

    def __init__(self, nodes, source, target, weight, is_distance=True):
        self.nodes = list(nodes)
        self.source = np.ascontiguousarray(source, dtype=np.int32)
        self.target = np.ascontiguousarray(target, dtype=np.int32)
        self.weight = np.ascontiguousarray(weight, dtype=np.float64)
        n = len(self.nodes)
        if not (self.source.shape == self.target.shape == self.weight.shape == (max(n - 1, 0),)):
            raise ValueError("source, target and weight must be three 1-D arrays of len(nodes) - 1 entries")
        if n > 1 and not ((self.source >= 0).all() and (self.source < self.target).all() and (self.target < n).all()):
            raise ValueError("an edge must join source < target, both indices into nodes")
        self.is_distance = bool(is_distance)

    @classmethod
    def from_dense(cls, matrix):
        """The tree of a filled ``SymMatrix``, in its current node order: every pair sorted by ``np.lexsort`` over (source,
        target, weight) -- the weight first, better first -- then Kruskal's algorithm with a union-find.  Host arithmetic: the
        statement ``Context.fill_tree`` is held to."""
        data = matrix._ordered()
        n = len(matrix)
        s, t = np.triu_indices(n, k=1)
        w = data[s, t]
        if np.isnan(w).any():
            raise TypeError("cannot build the tree of a matrix with unset edges")
        kept = _kruskal(n, s, t, w, matrix.is_distance)
        return cls(matrix.nodes, s[kept], t[kept], w[kept], is_distance=matrix.is_distance)

    def extended(self, nodes, rows, values):
        """This tree grown to ``nodes``: the host statement of ``tree_extend`` (arguments as ``SparseEdges.extended``).  MST(A + B) =
        MST(MST(A) + B): Kruskal's algorithm in the one total order over the stored edges, re-indexed, and the new pairs -- the
        order is strict and the re-indexing increasing, so the result is the canonical tree of the grown collection."""
        old_at, rows = _grown_positions(self.nodes, nodes, rows, "SingleLinkageTree.extended")
        n = len(nodes)
        src, tgt, w = _live_row_pairs(n, rows, values)
        if np.isnan(w).any():
            raise TypeError("cannot grow a tree by unset edges")
        s = np.concatenate([old_at[self.source], src])
        t = np.concatenate([old_at[self.target], tgt])
        w = np.concatenate([self.weight, w])
        kept = _kruskal(n, s, t, w, self.is_distance)
        if kept.shape[0] != max(n - 1, 0):
            raise ValueError("SingleLinkageTree.extended: the stored edges and the new pairs do not connect the nodes")
        return SingleLinkageTree(nodes, s[kept], t[kept], w[kept], is_distance=self.is_distance)

    def without(self, names):
        """Refused: a minimum spanning tree is not closed under vertex deletion -- the tree of the remaining genomes may need
        pairs this tree dropped because a removed genome offered a better path -- so removal needs a fill (``tree_de_novo`` over the
        remaining genomes; their stored tree edges may seed nothing: every pair among them is in question)."""
        raise NotImplementedError("SingleLinkageTree.without: a minimum spanning tree is not closed under vertex deletion; removing genomes "
                                  "needs a fill of the remaining ones (tree_de_novo)")

    def __len__(self):
        return int(self.weight.shape[0])

    def heights(self):
        """The merge heights: the weights in merge order (ascending on distances, descending on similarities)."""
        return self.weight.copy()

    def _labels(self, count):
        """Labels (the smallest member's index) of the components the first ``count`` edges span."""
        edges = SparseEdges(self.nodes, self.source[:count], self.target[:count], self.weight[:count], is_distance=self.is_distance)
        return edges.components()

    def cut(self, eps, strict=True):
        """The single-linkage clusters at ``eps`` as int32 labels, ``labels[g]`` = the smallest index of g's cluster (what
        :class:`Components` takes): the components of the pairs with ``weight < eps`` on distances, ``> eps`` on similarities;
        ``<=`` / ``>=`` with ``strict=False``.  The edges are in merge order, so the cut keeps a prefix of them."""
        w = self.weight
        if self.is_distance:
            keep = w < eps if strict else w <= eps
        else:
            keep = w > eps if strict else w >= eps
        return self._labels(int(keep.sum()))

    def cut_n(self, n_clusters):
        """``n_clusters`` clusters as labels: the first ``N - n_clusters`` merges of the total order.  Canonical, ties included; it
        is scikit-learn's single linkage for ``n_clusters`` wherever the two heights at the cut differ."""
        n = len(self.nodes)
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) or not 1 <= int(n_clusters) <= max(n, 1):
            raise ValueError(f"n_clusters must be an integer in 1..{max(n, 1)}, not {n_clusters!r}")
        return self._labels(max(n - int(n_clusters), 0))

    def linkage(self):
        """scipy's linkage matrix ``Z``, float64[N - 1, 4], of a distance tree: row i joins clusters ``Z[i, 0] < Z[i, 1]`` (a leaf's
        index, or N + the row that made the cluster) at ``Z[i, 2]`` into one of ``Z[i, 3]`` leaves."""
        if not self.is_distance:
            raise ValueError("linkage() takes a tree over distances (inverted() gives one)")
        n = len(self.nodes)
        z = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
        parent = list(range(n))
        ident, size = list(range(n)), [1] * n

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for i, (a, b, w) in enumerate(zip(self.source.tolist(), self.target.tolist(), self.weight.tolist())):
            ra, rb = find(a), find(b)
            if ra == rb:
                raise ValueError("the edges do not form a tree")
            z[i] = (min(ident[ra], ident[rb]), max(ident[ra], ident[rb]), w, size[ra] + size[rb])
            parent[rb] = ra
            ident[ra], size[ra] = n + i, size[ra] + size[rb]
        return z

    def leaves(self):
        """The dendrogram's leaf order as the reference computes it (``_get_tree_order``, matrix.py:673-686): indices into ``nodes``."""
        if len(self.nodes) < 2:
            return list(range(len(self.nodes)))
        return dendrogram(self.linkage(), no_plot=True, count_sort="descending")["leaves"]

    def __iter__(self):
        for i, j, w in zip(self.source.tolist(), self.target.tolist(), self.weight.tolist()):
            yield self.nodes[i], self.nodes[j], w

    def inverted(self):
        """distance <-> similarity: every weight becomes round(1 - w, 6), as ``SparseEdges.inverted``; the merge order is kept (the
        better weight stays the better one, and the tie-break does not look at it)."""
        return SingleLinkageTree(self.nodes, self.source, self.target, np.round(1.0 - self.weight, 6), is_distance=not self.is_distance)


def tree_de_novo(genomes, func, as_distance=True, slab_bytes=0):
    """The single-linkage dendrogram of ``matrix_de_novo(genomes, func, cpus, as_distance)`` as a :class:`SingleLinkageTree`, filled on
    the GPU by ``Context.fill_tree``: the dense matrix is never delivered, and beyond ``slab_bytes`` of HBM (0: automatic) never
    held; N - 1 edges cross PCIe.  ``func`` must be one of the six ``METRICS`` callables (no CPU route:
    ``SingleLinkageTree.from_dense(matrix_de_novo(...))`` serves another callable).  Several devices as ``edges_de_novo``
    (``MultiContext.fill_tree``: the same tree); under a launcher (``WORLD_SIZE`` > 1) it raises.  Every refusal comes before the
    first GPU call."""
    names, (src, tgt, val) = _de_novo_route(genomes, func, "tree_de_novo",
        lambda ctx, metric: ctx.fill_tree(metric, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: f"{len(genomes)} genomes -> {stats['n_edges']} tree edges from {record['genome_pairs']} pairs in "
                                      f"{stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): fill+rounds+D2H {fill_s:.3f} s (kernels "
                                      f"{stats['ms_total']:.3f} ms, rounds {stats.get('ms_rounds', 0.0):.3f} ms)",
        advice="for another callable: SingleLinkageTree.from_dense(matrix_de_novo(...))")
    return SingleLinkageTree(names, src, tgt, val, is_distance=as_distance)


# ---------------------------------------------------------------------------------------
# The table between the groups of a partition: count, sum, minimum and maximum of the pair values of every two groups
# ---------------------------------------------------------------------------------------
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
    index = {name: k for k, name in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("genome names must be distinct")
    members = _group_indices(names, index, groups)
    if len(members) < 1 or len(members) > BETWEEN_MAX_GROUPS:
        raise ValueError(f"between_de_novo: {len(members)} groups (1..{BETWEEN_MAX_GROUPS})")
    label = np.full(len(names), -1, dtype=np.int32)
    for a, idx in enumerate(members):
        taken = [i for i in idx if label[i] >= 0]
        if taken:
            raise ValueError(f"between_de_novo: genome '{names[taken[0]]}' is in groups {int(label[taken[0]])} and {a}")
        label[idx] = a
    if (label < 0).any():
        raise ValueError(f"between_de_novo: genome '{names[int(np.flatnonzero(label < 0)[0])]}' is in no group; the groups must cover the genomes")
    _, arrays = _de_novo_route(genomes, func, "between_de_novo",
        lambda ctx, metric: ctx.fill_between(metric, label, len(members), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: f"{len(genomes)} genomes in {len(members)} groups -> {len(members) * (len(members) + 1) // 2} entries from "
                                      f"{record['genome_pairs']} pairs in {stats['n_slabs']} slab(s) on {record['n_gpus']} device(s): "
                                      f"fill+reduce+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, reduction "
                                      f"{stats.get('ms_reduce', 0.0):.3f} ms)",
        advice="for another callable: GroupLinkage.from_dense(matrix_de_novo(...), groups)")
    return GroupLinkage([[names[i] for i in idx] for idx in members], *arrays, is_distance=as_distance)


AFFINITY_KINDS = ("mean", "nearest", "farthest")       # the three criteria of a nearest group, in the order of ``near_group``'s rows


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
        self.label = np.full(n, -1, dtype=np.int32)
        for b, group in enumerate(self.groups):
            for name in group:
                if name not in at:
                    raise KeyError(f"GroupAffinity: '{name}' of group {b} is no node")
                if self.label[at[name]] >= 0:
                    raise ValueError(f"GroupAffinity: '{name}' is in two groups")
                self.label[at[name]] = b
        if (self.label < 0).any():
            raise ValueError(f"GroupAffinity: '{self.nodes[int(np.flatnonzero(self.label < 0)[0])]}' is in no group")
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
        at = {name: k for k, name in enumerate(nodes)}
        n = len(nodes)
        label = np.full(n, -1, dtype=np.int64)
        for b, group in enumerate(groups):
            for name in group:
                if label[at[name]] >= 0:
                    raise ValueError(f"GroupAffinity: '{name}' is in two groups")
                label[at[name]] = b
        if (label < 0).any():
            raise ValueError(f"GroupAffinity: '{nodes[int(np.flatnonzero(label < 0)[0])]}' is in no group")
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
    index = {name: k for k, name in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("genome names must be distinct")
    members = _group_indices(names, index, groups)
    if len(members) < 1 or len(members) > BETWEEN_MAX_GROUPS:
        raise ValueError(f"affinity_de_novo: {len(members)} groups (1..{BETWEEN_MAX_GROUPS})")
    label = np.full(len(names), -1, dtype=np.int32)
    for a, idx in enumerate(members):
        taken = [i for i in idx if label[i] >= 0]
        if taken:
            raise ValueError(f"affinity_de_novo: genome '{names[taken[0]]}' is in groups {int(label[taken[0]])} and {a}")
        label[idx] = a
    if (label < 0).any():
        raise ValueError(f"affinity_de_novo: genome '{names[int(np.flatnonzero(label < 0)[0])]}' is in no group; the groups must cover the genomes")

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


# ---------------------------------------------------------------------------------------
# Growing a stored sparse result: new genomes against an edge list, a partition, a tree, k-nearest lists
# ---------------------------------------------------------------------------------------
def _extend_plan(stored_nodes, genomes, caller):
    """What ``edges_extend`` / ``components_extend`` / ``tree_extend`` check of their arguments, as ``matrix_extend`` does: distinct
    names, every stored node a genome (KeyError), the stored nodes in the genomes' relative order (ValueError).  Returns the genome
    names, ``old_at`` (the position among the genomes of every stored node: int64, strictly increasing) and the new positions."""
    if len(genomes) == 0:
        raise ValueError(f"{caller}: need at least 1 genome")
    names = [g.name for g in genomes]
    index = {name: k for k, name in enumerate(names)}
    if len(index) != len(names):
        raise ValueError(f"{caller}: genome names must be distinct")
    stranger = next((node for node in stored_nodes if node not in index), None)
    if stranger is not None:
        raise KeyError(f"{caller}: stored node '{stranger}' is not among the genomes: drop it first (without())")
    stored = set(stored_nodes)
    if len(stored) != len(stored_nodes):
        raise ValueError(f"{caller}: the stored nodes must be distinct")
    new_idx = [k for k, name in enumerate(names) if name not in stored]
    old_at, _ = _grown_positions(stored_nodes, names, new_idx, caller)
    return names, old_at, new_idx


def _guard_rows(ctx, metric, as_distance, old_at, verify):
    """The guard's refill: ``verify`` old genomes, chosen by ``matrix_extend``'s spread rule, against everyone through
    ``Context.fill_rows``.  Returns (their positions, ascending; their rows of values)."""
    n_verify = max(0, min(int(verify), int(old_at.shape[0])))
    checked = sorted({int(old_at[(i * old_at.shape[0]) // n_verify]) for i in range(n_verify)})
    if not checked:
        return checked, np.empty((0, ctx.n_genomes), dtype=np.float64)
    return checked, ctx.fill_rows(metric, checked, as_distance=as_distance)


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


def _extend_fill(plan, genomes, func, caller, as_distance, verify, guard, fill, log):
    """What the four ``*_extend`` routes share once some genomes are stored and some are new: the one pack and upload on one GPU
    (``upload_for_fills``: its refusals -- a callable outside ``METRICS``, a launcher -- come before any GPU call), the clock,
    ``_guard_rows``, the kind's ``guard(metric, checked, values)``, the rows fill ``fill(ctx, metric)`` -> ``(*arrays, stats)``,
    ``LAST_FILL`` and the log line (``_fill_done``).  Returns the arrays.  The early returns stay with the routes, in one order: every genome
    new -> de novo, nothing new -> the stored result re-laid without a GPU call."""
    names, old_at, new_idx = plan
    ctx, metric, _, record = upload_for_fills(genomes, func, caller, advice="for another callable: the extended() statement of the stored result "
                                                                            "takes any rows of values")
    import time
    t0 = time.perf_counter()
    checked, values = _guard_rows(ctx, metric, as_distance, old_at, verify)
    guard(metric, checked, values)
    *arrays, stats = fill(ctx, metric)
    _fill_done(stats, metric, names, record, t0, log, genome_pairs=int(stats["n_pairs"]), rows=len(new_idx), n_gpus=1)
    return arrays


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
            for g in old_at[(w <= threshold) if as_distance else (w >= threshold)].tolist():
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


def components_extend(components, genomes, func, threshold, strict=True, verify=4, as_distance=True, slab_bytes=0):
    """New genomes against a stored partition: the :class:`Components` over all of ``genomes`` that ``components_de_novo(genomes,
    func, threshold, as_distance, strict)`` would return, computing only the pairs that touch a genome ``components`` lacks
    (``Context.fill_rows_components``: the stored labels seed the forest).  Arguments, refusals and routes as ``edges_extend``.  The
    guard: a verified old genome and every old genome it passes the threshold with must share a stored label."""
    plan = names, old_at, new_idx = _extend_plan(components.nodes, genomes, "components_extend")
    if old_at.shape[0] == 0:
        return components_de_novo(genomes, func, threshold, as_distance=as_distance, strict=strict, slab_bytes=slab_bytes)
    seed = np.arange(len(names), dtype=np.int32)
    seed[old_at] = old_at[components.labels]
    if not new_idx:
        return Components(names, seed)

    def guard(metric, checked, values):
        for i, q in enumerate(checked):
            w = values[i, old_at]
            if as_distance:
                passing = w < threshold if strict else w <= threshold
            else:
                passing = w > threshold if strict else w >= threshold
            for g in old_at[passing].tolist():
                if g != q and seed[g] != seed[q]:
                    raise ValueError(f"pair ({names[min(q, g)]}, {names[max(q, g)]}): the {metric} fill gives {float(values[i, g])!r}, within the threshold "
                                     f"{threshold!r}, and the stored components keep the two apart: they were not filled with this metric and threshold "
                                     f"from these genomes")

    (labels,) = _extend_fill(plan, genomes, func, "components_extend", as_distance, verify, guard,
        lambda ctx, metric: ctx.fill_rows_components(metric, threshold, new_idx, seed_labels=seed, as_distance=as_distance, strict=strict,
                                                     slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: f"{len(new_idx)} new of {len(names)} genomes -> {stats['n_pairs']} pairs, {stats['n_components']} components in "
                                      f"{stats['n_slabs']} slab(s): guard+fill+union+labels {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)")
    return Components(names, labels)


def tree_extend(tree, genomes, func, verify=4, slab_bytes=0):
    """New genomes against a stored single-linkage tree: the :class:`SingleLinkageTree` over all of ``genomes`` that
    ``tree_de_novo(genomes, func, tree.is_distance)`` would return, edge for edge, computing only the pairs that touch a genome
    ``tree`` lacks (``Context.fill_rows_tree``: the stored edges seed the resident forest; MST(A + B) = MST(MST(A) + B)).  Arguments,
    refusals and routes as ``edges_extend``.  The guard: every stored edge that touches a verified old genome must carry exactly the
    refilled value.  Removing genomes is no such call: ``SingleLinkageTree.without`` says why."""
    plan = names, old_at, new_idx = _extend_plan(tree.nodes, genomes, "tree_extend")
    as_distance = tree.is_distance
    if old_at.shape[0] == 0:
        return tree_de_novo(genomes, func, as_distance=as_distance, slab_bytes=slab_bytes)
    src, tgt, weight = old_at[tree.source], old_at[tree.target], tree.weight
    if not new_idx:
        return SingleLinkageTree(names, src, tgt, weight, is_distance=as_distance)
    src, tgt, weight = _extend_fill(plan, genomes, func, "tree_extend", as_distance, verify,
        lambda metric, checked, values: _guard_edges(names, metric, checked, values, src, tgt, weight, "tree"),
        lambda ctx, metric: ctx.fill_rows_tree(metric, new_idx, seed=(src, tgt, weight), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True),
        lambda stats, record, fill_s: (
            f"{len(new_idx)} new of {len(names)} genomes -> {stats['n_pairs']} pairs, {stats['n_edges']} tree edges in {stats['n_slabs']} slab(s): "
            f"guard+fill+rounds+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms, rounds {stats.get('ms_rounds', 0.0):.3f} ms)"))
    return SingleLinkageTree(names, src, tgt, weight, is_distance=as_distance)


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
    with open(filepath, "w") as handle:
        handle.writelines(f"{source}\t{other}\t{weight:.6f}\n" for source, other, weight in found.inverted())
    return filepath


def nearest_from_file(filepath, names):
    """The distance :class:`NearestNeighbors` a ``nearest_<metric>.tsv`` holds, bit for bit: its nodes are the names that occur as
    sources in the file, in the order of ``names`` (the genomes in fill order; ``KeyError`` for a name they lack), and a similarity
    comes back as ``tree_from_file`` decodes it.  ``ValueError`` for a line that is no neighbour, sources whose lines are not together
    or come in another order than ``names``, an unequal number of lines per source, a count other than min(K, n - 1) (more than
    n - 1 lines for n sources, or none), or a target that is no source, the source itself, or listed twice."""
    index = {name: k for k, name in enumerate(names)}
    sources, lists = [], []
    with open(filepath, "r") as handle:
        for number, line in enumerate(handle, start=1):
            fields = line.rstrip("\n").split("\t")
            if len(fields) != 3:
                raise ValueError(f"{filepath}:{number}: expected source<TAB>target<TAB>similarity")
            for name in fields[:2]:
                if name not in index:
                    raise KeyError(f"{filepath}:{number}: '{name}' is not among the genomes")
            try:
                k = int(np.rint(float(fields[2]) * 1.0e6))
            except (ValueError, OverflowError):
                raise ValueError(f"{filepath}:{number}: '{fields[2]}' is no similarity") from None
            if not 0 <= k <= 1000000:
                raise ValueError(f"{filepath}:{number}: similarity {fields[2]} is outside [0, 1]")
            s = index[fields[0]]
            if not sources or sources[-1] != s:
                if sources and s <= sources[-1]:
                    raise ValueError(f"{filepath}:{number}: source '{fields[0]}' comes against the genomes' order (or its lines are not together): "
                                     "the file was written for another order")
                sources.append(s)
                lists.append([])
            lists[-1].append((index[fields[1]], (1000000 - k) / 1000000.0))
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


def tree_to_file(tree, filepath):
    """``tree_<metric>.tsv``: one ``source<TAB>target<TAB>similarity`` line per edge of a distance tree, in merge order; the weights
    inverted as for the adjacency file, "%.6f"."""
    with open(filepath, "w") as handle:
        handle.writelines(f"{source}\t{other}\t{weight:.6f}\n" for source, other, weight in tree.inverted())
    return filepath


def tree_from_file(filepath, names):
    """The distance :class:`SingleLinkageTree` a ``tree_<metric>.tsv`` holds, bit for bit: its nodes are the names that occur in the
    file, in the order of ``names`` (the genomes in fill order; ``KeyError`` for a name they lack), and a similarity of six places
    comes back as k = rint(sim * 10^6), distance = (10^6 - k) / 10^6 -- the tree fill's own decode, equal to the fill's
    round(1 - sim, 6).  ``ValueError`` for a line that is no edge, an edge whose source does not come before its target in that
    order, or a file that is no tree over its names."""
    index = {name: k for k, name in enumerate(names)}
    rows = []
    with open(filepath, "r") as handle:
        for number, line in enumerate(handle, start=1):
            fields = line.rstrip("\n").split("\t")
            if len(fields) != 3:
                raise ValueError(f"{filepath}:{number}: expected source<TAB>target<TAB>similarity")
            for name in fields[:2]:
                if name not in index:
                    raise KeyError(f"{filepath}:{number}: '{name}' is not among the genomes")
            k = int(np.rint(float(fields[2]) * 1.0e6))
            if not 0 <= k <= 1000000:
                raise ValueError(f"{filepath}:{number}: similarity {fields[2]} is outside [0, 1]")
            rows.append((index[fields[0]], index[fields[1]], (1000000 - k) / 1000000.0))
    present = sorted({g for s, t, _ in rows for g in (s, t)})
    at = {g: k for k, g in enumerate(present)}
    if len(rows) != max(len(present) - 1, 0):
        raise ValueError(f"{filepath}: {len(rows)} edges over {len(present)} names are no tree")
    bad = next(((s, t) for s, t, _ in rows if s >= t), None)
    if bad is not None:
        raise ValueError(f"{filepath}: edge ({names[bad[0]]}, {names[bad[1]]}) runs against the genomes' order: the file was written for another order")
    return SingleLinkageTree([names[g] for g in present], [at[s] for s, _, _ in rows], [at[t] for _, t, _ in rows], [w for _, _, w in rows],
                             is_distance=True)


def components_to_file(components, filepath):
    """``components_<metric>.tsv``: ``name<TAB>number`` in node order, number 1 for the largest group (``Components.groups()``'s order)."""
    number = [0] * len(components.nodes)
    for k, group in enumerate(components.group_indices(), start=1):
        for i in group.tolist():
            number[i] = k
    with open(filepath, "w") as handle:
        handle.writelines(f"{name}\t{k}\n" for name, k in zip(components.nodes, number))
    return filepath


def components_from_file(filepath):
    """The :class:`Components` a ``components_<metric>.tsv`` holds: its nodes in file order, every group labelled by its first member."""
    nodes, number = [], []
    with open(filepath, "r") as handle:
        for count, line in enumerate(handle, start=1):
            fields = line.rstrip("\n").split("\t")
            if len(fields) != 2 or not fields[1].isdigit():
                raise ValueError(f"{filepath}:{count}: expected name<TAB>number")
            nodes.append(fields[0])
            number.append(int(fields[1]))
    if len(set(nodes)) != len(nodes):
        raise ValueError(f"{filepath}: a name occurs twice")
    first = {}
    labels = [first.setdefault(k, g) for g, k in enumerate(number)]
    return Components(nodes, labels)


def edges_to_adjacency(edges, filepath, skip_zero=False, use_lib=True):
    """The bytes ``matrix_to_adjacency`` writes for the dense matrix restricted to these pairs (diagonal included).
    ``use_lib=False`` takes the Python formatter even when csrc/libpc_pack.so is there (same bytes)."""
    src, tgt, w = edges._adjacency_order()
    lib = _text_lib() if use_lib else None
    if lib is None or np.isnan(w).any():
        with open(filepath, "w") as handle:
            for i, j, x in zip(src.tolist(), tgt.tolist(), w.tolist()):
                if skip_zero and not x:
                    continue
                handle.write(f"{edges.nodes[i]}\t{edges.nodes[j]}\t{x:.6f}\n")
        return filepath
    import ctypes
    names = [name.encode() for name in edges.nodes]
    blob = b"".join(names)
    offsets = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in names], out=offsets[1:])
    step = 65536
    cap = step * (max((len(x) for x in names), default=0) * 2 + 32) + 1024
    buf = ctypes.create_string_buffer(cap)
    with open(filepath, "wb") as handle:
        for e0 in range(0, src.shape[0], step):
            n = min(step, src.shape[0] - e0)
            size = lib.pcp_format_edges(blob, offsets.ctypes.data, len(names), src[e0:].ctypes.data, tgt[e0:].ctypes.data, w[e0:].ctypes.data,
                                        n, 1 if skip_zero else 0, buf, cap)
            if size < 0:
                raise ValueError(f"{filepath}: edges {e0}..{e0 + n} do not fit their buffer (weights outside [0, 1]?)" if size == -1 else
                                 f"{filepath}: an edge names a node outside 0..{len(names) - 1}")
            handle.write(memoryview(buf)[:size])
    return filepath


def read_squareform(filepath):
    with open(filepath, "r") as handle:
        next(handle)
        for line in handle:
            fields = line.rstrip().split("\t")
            yield fields[0], [float(x) for x in fields[1:]]


def _read_rows(filepath):
    """(name, ndarray row) per line: the C parser when csrc/libpc_pack.so is there, else read_squareform."""
    lib = _text_lib()
    if lib is None:
        for name, row in read_squareform(filepath):
            yield name, np.asarray(row, dtype=np.float64)
        return
    with open(filepath, "rb") as handle:
        next(handle)
        for line in handle:
            line = line.rstrip()
            name, tab, rest = line.partition(b"\t")
            cap = rest.count(b"\t") + 1 if tab else 0
            row = np.empty(cap, dtype=np.float64)
            got = lib.pcp_parse_row(rest, len(rest), row.ctypes.data, cap) if cap else 0
            if got != cap:
                raise ValueError(f"{filepath}: could not parse the row of {name.decode()!r}")
            yield name.decode(), row


def matrix_from_squareform(filepath):
    names, rows, diagonal = [], [], set()
    for i, (target, row) in enumerate(_read_rows(filepath)):
        names.append(target)
        rows.append(row)
        diagonal.add(float(row[i]))
    matrix = SymMatrix(names, is_distance=_diagonal_kind(diagonal, len(diagonal)))
    n = len(names)
    data = matrix._data
    for i, row in enumerate(rows):
        values = np.asarray(row[:i + 1], dtype=np.float64)
        if values.size and not (values.min() >= 0.0 and values.max() <= 1.0):
            raise ValueError(f"weight not in [0.0, 1.0] on row {i}")
        values = np.round(values, 6)
        data[i, :i + 1] = values
        data[:i + 1, i] = values
    assert data.shape == (n, n)
    return matrix


def matrix_to_squareform(matrix, filepath, lower_triangle=False):
    lib = _text_lib() if isinstance(matrix, SymMatrix) else None
    data = matrix._ordered() if lib else None
    if lib is None or np.isnan(data).any():
        with open(filepath, "w") as handle:
            header = f"{len(matrix)}"
            if not lower_triangle:
                header += "\t" + "\t".join(matrix.nodes)
            handle.write(f"{header}\n")
            for i, (source, row) in enumerate(matrix.iterrows()):
                cells = row[:i + 1] if lower_triangle else row
                handle.write(f"{source}\t" + "\t".join([f"{x:.6f}" for x in cells]) + "\n")
        return filepath
    import ctypes
    n = len(matrix)
    data = np.ascontiguousarray(data, dtype=np.float64)
    cap = n * 24 + 1024
    buf = ctypes.create_string_buffer(cap)
    with open(filepath, "wb") as handle:
        header = f"{n}"
        if not lower_triangle:
            header += "\t" + "\t".join(matrix.nodes)
        handle.write(f"{header}\n".encode())
        for i, source in enumerate(matrix.nodes):
            size = lib.pcp_format_row(data[i].ctypes.data, i + 1 if lower_triangle else n, buf, cap)
            if size < 0:
                raise ValueError(f"{filepath}: the row of '{source}' does not fit its buffer (weights outside [0, 1]?)")
            handle.write(source.encode() + b"\t")
            handle.write(memoryview(buf)[:size])
    return filepath


def _get_tree_order(matrix):
    """Leaf order of a single-linkage dendrogram on distances (matrix.py:673-686)."""
    if not matrix.is_distance:
        matrix = matrix.extract_submatrix(matrix.nodes)
        matrix.invert()
    z = linkage(matrix.to_ndarray(condensed=True), method="single")
    return dendrogram(z, no_plot=True, get_leaves=True, count_sort="descending")["leaves"]
