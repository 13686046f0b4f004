"""What every accelerated route shares: the cached GPU contexts, the frame of a fill call, the checks of its arguments.

Owns the context registry (``get_context``, ``get_multi_context``, ``in_process_devices``), ``LAST_FILL`` (one dict, mutated
in place: what the last accelerated fill did), the frame of the ``*_de_novo`` routes (``upload_for_fills``, ``_de_novo_route``,
``_fill_done``) and of the ``*_extend`` routes (``_extend_plan``, ``_guard_rows``, ``_extend_fill``), and the checks of names and
groups they make before any GPU call (``_name_index``, ``_group_indices``, ``_partition_labels``, ``_ordered_positions``).
Below it lies only symmatrix.py; ``hip``, ``pack``, ``metrics`` and ``distributed`` are imported when a route first needs them.
"""

import logging
import os
import time

import numpy as np

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


def _metric_names(funcs, caller):
    """The metric names of ``funcs``, callables of ``METRICS``, in their order -- what the joint routes (``matrices_de_novo``,
    ``pairs_joint_de_novo``) check before any GPU call: ValueError for an empty list, a callable outside the six, a callable listed twice."""
    funcs = list(funcs)
    if not funcs:
        raise ValueError(f"{caller}: funcs is empty; name at least one of the six METRICS callables")
    names = []
    for k, func in enumerate(funcs):
        name = _metric_name(func)
        if name is None:
            raise ValueError(f"{caller}: funcs[{k}] is none of the six METRICS callables -- a joint fill runs on the GPU only and has no CPU route")
        if name in names:
            raise ValueError(f"{caller}: metric '{name}' is listed twice")
        names.append(name)
    return names


def _joint_upload(genomes, funcs, caller):
    """``upload_for_fills`` for the metrics of ``funcs`` (checked by ``_metric_names`` first): the residues go along when aai or peq is
    among them.  Returns ``(context, metric names, whether one joint fill serves them, genome names, record)``."""
    funcs = list(funcs)
    metrics = _metric_names(funcs, caller)
    aligned = [k for k, name in enumerate(metrics) if name in ("aai", "peq")]
    ctx, _, names, record = upload_for_fills(genomes, funcs[aligned[0] if aligned else 0], caller, advice="a joint fill has no CPU route")
    return ctx, metrics, bool(aligned), names, record


LAST_FILL = {}          # what the last accelerated matrix_de_novo did: the pipeline's log line reads it


def _packed_of(genomes):
    """The packed form of ``genomes``: the loader's own arrays when the list is exactly what the C loader produced
    (pack.load_tsv_genomes: untouched lazy genomes, all of them, in order), else a fresh pack of the objects."""
    from phamclust_amd.pack import pack_genomes, packed_behind
    return packed_behind(genomes) or pack_genomes(genomes)


def _slab_fill_context():
    """(context, devices used) of an edge-list, components, nearest-neighbours or tree fill: the ``MultiContext`` over the devices
    ``in_process_devices()`` names when there are several -- the four fills spread over them, a stretch of targets per device --
    else the one-GPU context (of the one device named, or the default device)."""
    devices = in_process_devices()
    if devices and len(devices) > 1:
        return get_multi_context(devices), len(devices)
    return get_context(devices[0] if devices else None), 1


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
    fill_s = time.perf_counter() - t0
    LAST_FILL.clear()
    LAST_FILL.update(stats, metric=metric, n_genomes=len(names), rank=0, pack_s=record["pack_s"], upload_s=record["upload_s"], fill_s=fill_s, **own)
    logging.debug(log(stats, record, fill_s))


def _de_novo_route(genomes, func, caller, fill, log, advice="the dense route, matrix_de_novo, serves another callable", several=True):
    """The frame the ``*_de_novo`` routes share: ``upload_for_fills`` over the devices at hand (``advice``: its refusal's; ``several=False``: a
    one-GPU fill, ``placement_de_novo``'s), the clock, ``fill(ctx, metric)`` -> ``(*arrays, stats)``, ``LAST_FILL`` and the log line
    (``_fill_done``).  Returns ``(names, arrays)``."""
    ctx, metric, names, record = upload_for_fills(genomes, func, caller, several=several, advice=advice)
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


def _name_index(names):
    """name -> position among the genomes; ValueError when a name occurs twice."""
    index = {name: k for k, name in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("genome names must be distinct")
    return index


def _partition_labels(names, groups, caller, max_groups):
    """``groups`` (as ``_group_indices`` takes them) as a partition of the genomes ``names``: ``(members, label)`` -- the groups as
    ascending index lists and int32 ``label[g]`` = the group of genome g.  ValueError for a name twice, fewer than 1 or more than
    ``max_groups`` groups, a genome in two groups or in none, besides ``_group_indices``' refusals."""
    members = _group_indices(names, _name_index(names), groups)
    if len(members) < 1 or len(members) > max_groups:
        raise ValueError(f"{caller}: {len(members)} groups (1..{max_groups})")
    label = np.full(len(names), -1, dtype=np.int32)
    for a, idx in enumerate(members):
        taken = [i for i in idx if label[i] >= 0]
        if taken:
            raise ValueError(f"{caller}: genome '{names[taken[0]]}' is in groups {int(label[taken[0]])} and {a}")
        label[idx] = a
    if (label < 0).any():
        raise ValueError(f"{caller}: genome '{names[int(np.flatnonzero(label < 0)[0])]}' is in no group; the groups must cover the genomes")
    return members, label


def _ordered_positions(stored_nodes, index, caller):
    """``old_at[k]`` = ``index[stored_nodes[k]]`` as int64, which must be strictly increasing: ValueError for stored nodes that come in
    another order in the grown collection."""
    old_at = np.fromiter((index[node] for node in stored_nodes), dtype=np.int64, count=len(stored_nodes))
    if old_at.shape[0] > 1 and not (np.diff(old_at) > 0).all():
        k = int(np.flatnonzero(np.diff(old_at) <= 0)[0])
        raise ValueError(f"{caller}: stored nodes '{stored_nodes[k]}' and '{stored_nodes[k + 1]}' come in another order in the grown collection: "
                         "orientation and tie order follow the order, so a result can only be grown in its own order")
    return old_at


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
    return names, _ordered_positions(stored_nodes, index, caller), new_idx


def _guard_rows(ctx, metric, as_distance, old_at, verify):
    """The guard's refill: ``verify`` old genomes, chosen by ``matrix_extend``'s spread rule, against everyone through
    ``Context.fill_rows``.  Returns (their positions, ascending; their rows of values)."""
    n_verify = max(0, min(int(verify), int(old_at.shape[0])))
    checked = sorted({int(old_at[(i * old_at.shape[0]) // n_verify]) for i in range(n_verify)})
    if not checked:
        return checked, np.empty((0, ctx.n_genomes), dtype=np.float64)
    return checked, ctx.fill_rows(metric, checked, as_distance=as_distance)


def _extend_fill(plan, genomes, func, caller, as_distance, verify, guard, fill, log):
    """What the four ``*_extend`` routes share once some genomes are stored and some are new: the one pack and upload on one GPU
    (``upload_for_fills``: its refusals -- a callable outside ``METRICS``, a launcher -- come before any GPU call), the clock,
    ``_guard_rows``, the kind's ``guard(metric, checked, values)``, the rows fill ``fill(ctx, metric)`` -> ``(*arrays, stats)``,
    ``LAST_FILL`` and the log line (``_fill_done``).  Returns the arrays.  The early returns stay with the routes, in one order: every genome
    new -> de novo, nothing new -> the stored result re-laid without a GPU call."""
    names, old_at, new_idx = plan
    ctx, metric, _, record = upload_for_fills(genomes, func, caller, advice="for another callable: the extended() statement of the stored result "
                                                                            "takes any rows of values")
    t0 = time.perf_counter()
    checked, values = _guard_rows(ctx, metric, as_distance, old_at, verify)
    guard(metric, checked, values)
    *arrays, stats = fill(ctx, metric)
    _fill_done(stats, metric, names, record, t0, log, genome_pairs=int(stats["n_pairs"]), rows=len(new_idx), n_gpus=1)
    return arrays
