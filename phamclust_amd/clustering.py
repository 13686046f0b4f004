"""Agglomerative clustering of a distance ``SymMatrix`` (the reference's clustering.py:4-51 contract).

scikit-learn's ``AgglomerativeClustering`` on the precomputed matrix does the work, as in the reference.
The hand-off is what differs: ``to_ndarray()`` is one fancy-index of the array the GPU fill produced, and the
members of each label are gathered with numpy instead of per-node Python dict traffic.
"""

import numpy as np
from sklearn.cluster import AgglomerativeClustering


def hierarchical_clustering(matrix, linkage, eps=None, n_clusters=None):
    """Sub-matrices of the clusters, largest first.  Give either ``eps`` (distance threshold) or ``n_clusters``."""
    if len(matrix) == 1:
        return [matrix]
    if not matrix.is_distance:
        raise ValueError("matrix must be a distance matrix")
    if eps is None and not n_clusters:
        raise ValueError("need either threshold or n_clusters to proceed")
    if eps and n_clusters:
        raise ValueError("threshold and n_clusters are mutually exclusive")
    labels = AgglomerativeClustering(metric="precomputed", linkage=linkage, distance_threshold=eps,
                                     n_clusters=n_clusters).fit_predict(matrix.to_ndarray())
    nodes = np.asarray(matrix.nodes, dtype=object)
    # clusters in order of first appearance of their label, as a dict keyed by label would give
    _, first = np.unique(labels, return_index=True)
    parts = [matrix.extract_submatrix(nodes[labels == labels[i]].tolist()) for i in sorted(first)]
    return sorted(parts, reverse=True)


def cluster_by_component(groups, submatrix_of, linkage, eps, nodes=None):
    """``hierarchical_clustering`` component by component.  ``groups``: the connected components of the graph {d < eps} as lists
    of node names, each in node order (``Components.groups()``); ``submatrix_of(names)``: the distance ``SymMatrix`` over one group.
    A cluster cut at ``eps`` never spans two components -- a merge at height h < eps holds a pair with d <= h, for ``single``,
    ``average`` and ``complete`` alike -- so each group of two or more is clustered alone and a group of one is its own matrix.
    The parts come back as the dense route orders them: by first appearance in the node order, i.e. by the position of a part's
    smallest member, then ``sorted(..., reverse=True)``, which is stable.  ``nodes``: that node order; None: the names' sorted
    order, which is the pipeline's (genomes are read sorted by name) -- a group that is not ascending by name is then refused."""
    if linkage == "ward":
        raise ValueError("ward's merge height is not bounded below by a pair distance: its clusters can span components")
    if eps is None:
        raise ValueError("clustering by component needs a distance threshold")
    from phamclust_amd.matrix import SymMatrix
    groups = [list(names) for names in groups]
    if nodes is None:
        if any(a >= b for names in groups for a, b in zip(names, names[1:])):
            raise ValueError("cluster_by_component: the groups are not in name order; give the node order as nodes=")
        first = min                                          # a part's first node in the node order
    else:
        position = {node: k for k, node in enumerate(nodes)}
        first = lambda names: min(position[node] for node in names)      # noqa: E731
    parts = []
    for names in groups:
        if len(names) == 1:
            single = SymMatrix(nodes=names, is_distance=True)
            single.set_weight(names[0], names[0], 0.0)
            parts.append(single)
        else:
            parts.extend(hierarchical_clustering(submatrix_of(names), linkage, eps=eps))
    parts.sort(key=lambda part: first(part.nodes))
    return sorted(parts, reverse=True)


def hierarchical_clustering_de_novo(genomes, func, linkage, eps=None, cpus=1, n_clusters=None):
    """``hierarchical_clustering(matrix_de_novo(genomes, func, cpus), linkage, eps=eps)`` without the N x N matrix.

    The connected components of {d < eps} come from one components fill on the GPU (``Context.fill_components``: N labels cross
    PCIe); every component of two or more genomes is then filled by ONE groups fill over the same upload (``Context.fill_groups``:
    the components' condensed triangles) -- its genomes in their original relative order, so every pair keeps its orientation and its
    value bit for bit (aai included) -- and clustered alone (``cluster_by_component``).  One pack, one upload, two fills, whatever the
    number of components; memory is the sum of n_c^2 over the components, not N^2.

    The result equals the dense route's as a list of node lists, order included: always for ``single``; for ``average`` and
    ``complete`` wherever the dense route's own result does not hinge on how scipy breaks a tie between two merges (that is every
    committed fixture).  ``ward`` and ``n_clusters=`` raise ``ValueError``: ward's height is not bounded below by a pair distance,
    and a cluster count is a property of the whole dendrogram.  ``func`` must be one of the six ``METRICS`` callables; one GPU.
    ``cpus`` is accepted for signature compatibility only (nothing runs on a worker pool).  ``matrix.LAST_FILL`` afterwards holds the
    groups fill's stats (``genome_pairs`` = the pairs it filled, ``groups``) beside ``n_components`` / ``n_edges`` / ``n_slabs`` /
    ``ms_components`` of the components fill."""
    if n_clusters:
        raise ValueError("hierarchical_clustering_de_novo cuts at a distance threshold: n_clusters needs the whole dendrogram (the dense route, or "
                         "for single linkage tree_de_novo(...).cut_n)")
    if linkage == "ward":
        raise ValueError("hierarchical_clustering_de_novo: ward's merge height is not bounded below by a pair distance (the dense route serves it)")
    if eps is None:
        raise ValueError("need a distance threshold (eps) to proceed")
    import time
    from phamclust_amd import matrix as M
    ctx, metric, names, record = M.upload_for_fills(genomes, func, "hierarchical_clustering_de_novo")
    t0 = time.perf_counter()
    labels, cc = ctx.fill_components(metric, eps, as_distance=True, strict=True, want_stats=True)
    components = M.Components(names, labels)
    groups = [g for g in components.group_indices() if len(g) > 1]
    condensed, stats = ctx.fill_groups(metric, groups, as_distance=True, want_stats=True)
    M.LAST_FILL.clear()                                  # the groups fill's counts; the components fill's under its own names
    M.LAST_FILL.update(stats, metric=metric, n_genomes=len(names), genome_pairs=int(stats["n_pairs"]), groups=len(groups), n_gpus=1, rank=0,
                       n_components=cc["n_components"], n_edges=cc["n_edges"], n_slabs=cc["n_slabs"], ms_components=cc["ms_total"],
                       pack_s=record["pack_s"], upload_s=record["upload_s"], fill_s=time.perf_counter() - t0)
    filled = {names[int(g[0])]: M.SymMatrix.from_condensed([names[i] for i in g.tolist()], values, is_distance=True) for g, values in zip(groups, condensed)}
    return cluster_by_component(components.groups(), lambda group: filled[group[0]], linkage, eps, nodes=names)
