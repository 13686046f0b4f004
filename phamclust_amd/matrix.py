"""``matrix_de_novo`` and the matrix files: the reference's matrix.py surface over ndarray storage.

``matrix_de_novo(genomes, func, cpus, as_distance=True)`` is the drop-in boundary
(reference matrix.py:432-497, called from scripts/phamclust.py:258).  When ``func`` is one
of the six ``METRICS`` callables the whole N x N fill runs on the GPU through
``libphamclust_hip.so`` (one upload, one ``pc_fill``); any other callable takes the generic
per-pair loop with the reference's semantics.  There is no CPU fallback for the six
metrics: a missing library or a failing call raises.

Owns the routes whose results are ``SymMatrix``es (``matrix_de_novo``, ``matrices_de_novo``, ``matrix_extend``, ``submatrices_de_novo``) and the text
I/O of the dense matrix with its C formatter (``_text_lib``; ``edges_to_adjacency`` writes the same bytes through it, so it
lives here).  ``SymMatrix`` itself is symmatrix.py's, what the accelerated routes share is routes.py's, and every result that
is no dense matrix has a module under results/ -- all of their names stay readable from here.
"""

import logging
import os
import time

import numpy as np

from phamclust_amd.symmatrix import SymMatrix, _get_tree_order, _square_matrix  # noqa: F401
from phamclust_amd.routes import (LAST_FILL, _CONTEXTS, _de_novo_route, _extend_fill, _extend_plan, _fill_done, _group_indices,  # noqa: F401
                                  _guard_rows, _joint_upload, _metric_name, _metric_names, _name_index, _packed_of, _slab_fill_context,
                                  default_device, get_context, get_multi_context, in_process_devices, upload_for_fills)
from phamclust_amd.results._common import _grown_positions, _live_row_pairs, _positions_without  # noqa: F401
from phamclust_amd.results.edges import SparseEdges, _guard_edges, edges_de_novo, edges_extend, merge_edge_lists  # noqa: F401
from phamclust_amd.results.pairs import pairs_de_novo, pairs_joint_de_novo  # noqa: F401
from phamclust_amd.results.components import (Components, components_de_novo, components_extend, components_from_file,  # noqa: F401
                                              components_to_file)
from phamclust_amd.results.neighbors import (NEAREST_MAX_K, NearestNeighbors, _guard_neighbors, nearest_from_file, nearest_to_file,  # noqa: F401
                                             neighbors_de_novo, neighbors_extend)
from phamclust_amd.results.tree import SingleLinkageTree, _kruskal, tree_de_novo, tree_extend, tree_from_file, tree_to_file  # noqa: F401
from phamclust_amd.results.distribution import (HIST_BINS, PairDistribution, distribution_de_novo, distribution_extend,  # noqa: F401
                                                distribution_from_file, distribution_to_file)
from phamclust_amd.results.linkage import (BETWEEN_MAX_GROUPS, MILLION, _EMPTY_HI, _EMPTY_LO, GroupLinkage, between_de_novo,  # noqa: F401
                                           between_extend, between_from_file, between_to_file)
from phamclust_amd.results.affinity import (AFFINITY_KINDS, _AFFINITY_COLUMNS, GroupAffinity, affinity_de_novo, affinity_from_file,  # noqa: F401
                                            affinity_to_file)
from phamclust_amd.results.placement import (GroupPlacement, GrownOwn, _PLACEMENT_COLUMNS, own_similarity_text, placement_de_novo,  # noqa: F401
                                             placement_from_file, placement_report, placement_to_file, stored_fit_from_file)


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


def matrices_de_novo(genomes, funcs, cpus, as_distance=True):
    """``{metric name: matrix_de_novo(genomes, func, cpus, as_distance) for func in funcs}`` off ONE pack, ONE upload and -- when aai or
    peq is among ``funcs`` -- ONE joint fill (``Context.fill_joint``): one plan and one alignment pass deliver every metric asked for,
    where ``matrix_de_novo`` per metric aligns again for each of aai and peq.  Every matrix equals ``matrix_de_novo``'s cell for cell,
    bit for bit.  With only set metrics among ``funcs`` (gcs / jc / pocp / af) there is no alignment pass to share: one upload, then the
    single fills.  ``funcs`` are ``METRICS`` callables, each at most once; ``cpus`` is accepted for signature compatibility.  One GPU, as
    ``submatrices_de_novo``: under a launcher (``WORLD_SIZE`` > 1) it raises.  Every refusal -- an empty list, a callable outside
    ``METRICS``, a callable listed twice, a launcher -- comes before the first GPU call.  ``LAST_FILL`` reports the joint fill (``fills``
    = 1, ``metrics``) or, without one, the sums over the single fills."""
    ctx, metrics, joint, names, record = _joint_upload(genomes, funcs, "matrices_de_novo")
    t0 = time.perf_counter()
    if joint:
        arrays, stats = ctx.fill_joint(metrics, as_distance=as_distance, want_stats=True)
    else:
        arrays, stats = {}, None
        for name in metrics:
            arrays[name], one = ctx.fill(name, as_distance=as_distance, want_stats=True)
            stats = one if stats is None else dict(stats, ms_total=stats["ms_total"] + one["ms_total"], ms_reduce=stats["ms_reduce"] + one["ms_reduce"])
    _fill_done(stats, "+".join(metrics), names, record, t0,
               lambda stats, record, fill_s: f"{len(names)} genomes -> {record['genome_pairs']} edges x {len(metrics)} metrics ({', '.join(metrics)}) "
                                             f"on one device: {'one joint fill' if joint else 'single fills'}+D2H {fill_s:.3f} s "
                                             f"(kernels {stats['ms_total']:.3f} ms)",
               genome_pairs=record["genome_pairs"], n_gpus=1, metrics=tuple(metrics), fills=1 if joint else len(metrics))
    return {name: SymMatrix.from_condensed(names, arrays[name], is_distance=as_distance) for name in metrics}


def _row_adjacency(source, targets, func, distance):
    """One worker task of the generic path: ``source`` against a run of targets."""
    return [calculate_adjacency(source, target, func, distance) for target in targets]


def _pairs_adjacency(pairs, func, distance):
    """One worker task of matrix_extend's generic path: a run of (source, target) pairs."""
    return [calculate_adjacency(source, target, func, distance) for source, target in pairs]


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
    index = _name_index(names)
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
    members = _group_indices(names, _name_index(names), groups)
    ctx, metric, names, record = upload_for_fills(genomes, func, "submatrices_de_novo")
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
