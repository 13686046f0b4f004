"""The components: single-linkage clusters at a threshold as one label per genome, without the dense matrix or an edge list.

Owns ``Components``, its routes ``components_de_novo`` and ``components_extend``, and its file (``components_to_file`` /
``components_from_file``)."""

import numpy as np

from phamclust_amd.routes import _de_novo_route, _extend_fill, _extend_plan
from phamclust_amd.results._common import _grown_positions, _live_row_pairs, _passes, _positions_without, _smallest_member_labels


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
        old_at, rows = _grown_positions(self.nodes, nodes, rows, "Components.extended")
        src, tgt, w = _live_row_pairs(len(nodes), rows, values)
        keep = _passes(w, threshold, is_distance, strict)
        return Components(nodes, _smallest_member_labels(len(nodes), np.concatenate([old_at[self.labels], src[keep]]),
                                                         np.concatenate([old_at, tgt[keep]])))

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
            for g in old_at[_passes(values[i, old_at], threshold, as_distance, strict)].tolist():
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
