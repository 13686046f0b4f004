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

    The connected components of {d < eps} come from one components fill on the GPU (``components_de_novo(genomes, func, eps,
    strict=True)``: N labels cross PCIe); each component of two or more genomes is then filled by a ``matrix_de_novo`` of its own --
    its genomes in their original relative order, so every pair keeps its orientation and its value bit for bit (aai included) -- and
    clustered alone (``cluster_by_component``).  Memory is the sum of n_c^2 over the components, not N^2.

    The result equals the dense route's as a list of node lists, order included: always for ``single``; for ``average`` and
    ``complete`` wherever the dense route's own result does not hinge on how scipy breaks a tie between two merges (that is every
    committed fixture).  ``ward`` and ``n_clusters=`` raise ``ValueError``: ward's height is not bounded below by a pair distance,
    and a cluster count is a property of the whole dendrogram.  ``func`` must be one of the six ``METRICS`` callables; one GPU."""
    if n_clusters:
        raise ValueError("hierarchical_clustering_de_novo cuts at a distance threshold: n_clusters needs the whole dendrogram (the dense route)")
    if linkage == "ward":
        raise ValueError("hierarchical_clustering_de_novo: ward's merge height is not bounded below by a pair distance (the dense route serves it)")
    if eps is None:
        raise ValueError("need a distance threshold (eps) to proceed")
    from phamclust_amd.matrix import components_de_novo, matrix_de_novo
    components = components_de_novo(genomes, func, eps, as_distance=True, strict=True)
    by_name = {g.name: g for g in genomes}
    return cluster_by_component(components.groups(), lambda names: matrix_de_novo([by_name[name] for name in names], func, cpus, as_distance=True),
                                linkage, eps, nodes=[g.name for g in genomes])
