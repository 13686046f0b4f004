"""The pair list: the values of the pairs a caller names, without the dense matrix.

Owns ``pairs_de_novo`` (and ``pairs_joint_de_novo``, several metrics of the same list off one alignment pass), the bulk form of the reference's most basic interface -- ``METRICS[metric](source, target)`` per pair
(cli.py:30-35) -- over ``Context.fill_pairs``: one pack, one upload, one call for any number of listed pairs, each oriented as
written.  ``SparseEdges.rescored`` and the ``prefilter`` of ``edges_de_novo`` (results/edges.py) are built on the same call."""

import time

import numpy as np

from phamclust_amd.routes import _fill_done, _joint_upload, _name_index, upload_for_fills


def _pair_indices(names, index, pairs, caller):
    """``pairs`` -- a sequence of (name or index, name or index), or an integer array of shape (L, 2) -- as two int32 arrays of
    positions among the genomes.  KeyError for an unknown name, IndexError for an index outside the list, ValueError for an entry
    that is no pair."""
    if isinstance(pairs, np.ndarray) and pairs.dtype.kind in "iu":
        if pairs.ndim != 2 or pairs.shape[1] != 2:
            raise ValueError(f"{caller}: an index array of pairs must have shape (L, 2), not {pairs.shape}")
        bad = np.flatnonzero(((pairs < 0) | (pairs >= len(names))).any(axis=1))
        if bad.shape[0]:
            k = int(bad[0])
            raise IndexError(f"{caller}: pair {k}: genome index {int(pairs[k][(pairs[k] < 0) | (pairs[k] >= len(names))][0])} is outside 0..{len(names) - 1}")
        return np.ascontiguousarray(pairs[:, 0], dtype=np.int32), np.ascontiguousarray(pairs[:, 1], dtype=np.int32)
    src, tgt = [], []
    for k, pair in enumerate(pairs):
        if isinstance(pair, (str, bytes)) or len(pair) != 2:
            raise ValueError(f"{caller}: entry {k} is no pair of two genomes: {pair!r}")
        for member, out in zip(pair, (src, tgt)):
            if isinstance(member, (int, np.integer)) and not isinstance(member, bool):
                if not 0 <= int(member) < len(names):
                    raise IndexError(f"{caller}: pair {k}: genome index {int(member)} is outside 0..{len(names) - 1}")
                out.append(int(member))
            elif member in index:
                out.append(index[member])
            else:
                raise KeyError(f"{caller}: pair {k}: '{member}' is not among the genomes")
    return np.asarray(src, dtype=np.int32), np.asarray(tgt, dtype=np.int32)


def pairs_de_novo(genomes, func, pairs, as_distance=True):
    """``[func(genomes[s], genomes[t], as_distance) for s, t in pairs]`` as a float64 array in the caller's order, filled on the GPU
    by ONE pair-list fill (``Context.fill_pairs``) after one pack and one upload.  ``pairs`` is a sequence of (name or index, name
    or index) -- or an integer array of shape (L, 2) -- and every entry is ORIENTED as written: its first genome is the reference's
    ``source``.  With the first genome earlier in ``genomes`` than the second the value is ``matrix_de_novo``'s cell bit for bit;
    reversed, under aai / peq, it is the reference's value for the reversed call (the four set metrics are symmetric).  A genome
    against itself gives the diagonal, ``1.0 - as_distance``; a pair may be listed any number of times.  ``func`` must be one of
    the six ``METRICS`` callables (no CPU route: for another callable call it per pair).  One GPU, as ``submatrices_de_novo``: under
    a launcher (``WORLD_SIZE`` > 1) it raises.  Every refusal -- an unknown name, an index outside the list, a callable outside
    ``METRICS``, a launcher -- comes before the first GPU call."""
    names = [g.name for g in genomes]
    src, tgt = _pair_indices(names, _name_index(names), pairs, "pairs_de_novo")
    ctx, metric, names, record = upload_for_fills(genomes, func, "pairs_de_novo", advice="for another callable: call it per pair")
    t0 = time.perf_counter()
    values, stats = ctx.fill_pairs(metric, src, tgt, as_distance=as_distance, want_stats=True)
    _fill_done(stats, metric, names, record, t0,
               lambda stats, record, fill_s: f"{len(names)} genomes, {src.shape[0]} listed pairs ({stats['n_pairs']} off the diagonal) of "
                                             f"{record['genome_pairs']} on one device: sort+fill+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)",
               genome_pairs=int(stats["n_pairs"]), listed=int(src.shape[0]), n_gpus=1)
    return values


def pairs_joint_de_novo(genomes, funcs, pairs, as_distance=True):
    """``{metric name: pairs_de_novo(genomes, func, pairs, as_distance) for func in funcs}`` off ONE pack, ONE upload and -- when aai or
    peq is among ``funcs`` -- ONE joint pair-list fill (``Context.fill_pairs_joint``): one plan and one alignment pass for every metric
    asked for.  ``pairs_de_novo``'s contract for names and indices, orientation (every entry as written, under every metric), repeats
    and the diagonal; every array equals ``pairs_de_novo``'s bit for bit.  With only set metrics among ``funcs`` there is no alignment
    pass to share: one upload, then the single fills.  ``funcs`` are ``METRICS`` callables, each at most once.  One GPU; every refusal
    -- ``pairs_de_novo``'s, an empty list, a callable outside ``METRICS``, a callable listed twice -- comes before the first GPU call."""
    names = [g.name for g in genomes]
    src, tgt = _pair_indices(names, _name_index(names), pairs, "pairs_joint_de_novo")
    ctx, metrics, joint, names, record = _joint_upload(genomes, funcs, "pairs_joint_de_novo")
    t0 = time.perf_counter()
    if joint:
        arrays, stats = ctx.fill_pairs_joint(metrics, src, tgt, as_distance=as_distance, want_stats=True)
    else:
        arrays, stats = {}, None
        for name in metrics:
            arrays[name], one = ctx.fill_pairs(name, src, tgt, as_distance=as_distance, want_stats=True)
            stats = one if stats is None else dict(stats, ms_total=stats["ms_total"] + one["ms_total"], ms_reduce=stats["ms_reduce"] + one["ms_reduce"])
    _fill_done(stats, "+".join(metrics), names, record, t0,
               lambda stats, record, fill_s: f"{len(names)} genomes, {src.shape[0]} listed pairs ({stats['n_pairs']} off the diagonal) of "
                                             f"{record['genome_pairs']} x {len(metrics)} metrics ({', '.join(metrics)}) on one device: "
                                             f"sort+{'one joint fill' if joint else 'single fills'}+D2H {fill_s:.3f} s (kernels {stats['ms_total']:.3f} ms)",
               genome_pairs=int(stats["n_pairs"]), listed=int(src.shape[0]), n_gpus=1, metrics=tuple(metrics), fills=1 if joint else len(metrics))
    return {name: arrays[name] for name in metrics}
