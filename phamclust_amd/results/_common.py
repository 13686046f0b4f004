"""Host helpers the result classes share: growing and shrinking a stored result's node list, the pairs of a rows array, the
threshold predicate, the components' labels, and the ``source<TAB>target<TAB>similarity`` files of the nearest-neighbours
and tree results.  Host arithmetic only: no GPU call starts here."""

import numpy as np

from phamclust_amd.routes import _ordered_positions


def _passes(w, threshold, is_distance, strict=False):
    """Which weights ``w`` are within ``threshold``: ``<=`` on distances, ``>=`` on similarities; ``<`` / ``>`` with ``strict``."""
    if is_distance:
        return w < threshold if strict else w <= threshold
    return w > threshold if strict else w >= threshold


def _smallest_member_labels(n, src, tgt):
    """The connected components of the graph over ``n`` nodes with the edges (src[e], tgt[e]) as int32 labels, ``labels[g]`` = the
    smallest index of g's component (``scipy.sparse.csgraph``)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    graph = coo_matrix((np.ones(src.shape[0], dtype=np.int8), (src, tgt)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    smallest = np.full(int(comp.max()) + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.int32)


def _similarity_lines(filepath, index):
    """The lines of a ``source<TAB>target<TAB>similarity`` file as ``(line number, source, target, millionths)``: ``index`` maps a
    name to its position (KeyError for a name it lacks), the similarity comes back as k = rint(sim * 10^6) -- a distance is then
    (10^6 - k) / 10^6, the fills' own round(1 - sim, 6).  ValueError for a line of another shape or a value outside [0, 1]."""
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
            yield number, index[fields[0]], index[fields[1]], k


def _similarity_lines_to_file(result, filepath):
    """One ``source<TAB>target<TAB>similarity`` line per (source, target, weight) a distance result yields, in its order; the
    weights inverted as for the adjacency file, "%.6f"."""
    with open(filepath, "w") as handle:
        handle.writelines(f"{source}\t{other}\t{weight:.6f}\n" for source, other, weight in result.inverted())
    return filepath


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
    old_at = _ordered_positions(stored_nodes, index, caller)
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
