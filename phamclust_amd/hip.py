"""ctypes binding of ``libphamclust_hip.so`` (C-ABI: ``include/phamclust_hip.h``).

This is the only way the package computes anything: there is no CPU fallback.  If the
library is missing or a call fails, the error is raised, never papered over.
"""

import ctypes
import os
import weakref

import numpy as np

# PHAMCLUST_NATIVE_VARIANT=hooks loads the twin compiled with -DPC_TEST_HOOKS (fault injection; one GPU test runs on it); any other
# name but "asan" (the host libraries' sanitized twins) loads csrc/libphamclust_hip_<name>.so -- A/B of two builds in one GPU call
_variant = os.environ.get("PHAMCLUST_NATIVE_VARIANT", "")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                        f"libphamclust_hip_{_variant}.so" if _variant not in ("", "asan") else "libphamclust_hip.so")
METRIC_IDS = {"gcs": 0, "jc": 1, "pocp": 2, "af": 3, "aai": 4, "peq": 5, "aai_ppos": 6}

_u8p = ctypes.POINTER(ctypes.c_uint8)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_f64p = ctypes.POINTER(ctypes.c_double)


class HipLibraryError(RuntimeError):
    """The HIP library is missing, or one of its entry points returned an error."""


class PcPacked(ctypes.Structure):
    _fields_ = [("n_genomes", ctypes.c_int32), ("n_phams", ctypes.c_int32),
                ("words_per_row", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("bitmap", _u64p), ("nph", _i32p), ("ngen", _i32p), ("tlen", _i64p),
                ("gene_off", _i64p), ("gene_pham", _i32p), ("seq_off", _i64p), ("residues", _u8p)]


class PcStats(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int64), ("n_alignments", ctypes.c_int64), ("n_cells", ctypes.c_int64),
                ("n_tasks", ctypes.c_int64), ("n_residue_bytes", ctypes.c_int64),
                ("n_align_launches", ctypes.c_int32), ("n_chunks", ctypes.c_int32),
                ("ms_total", ctypes.c_float), ("ms_plan", ctypes.c_float), ("ms_align", ctypes.c_float),
                ("ms_reduce", ctypes.c_float), ("n_distinct_alignments", ctypes.c_int64), ("n_distinct_cells", ctypes.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PcSetInputs(ctypes.Structure):
    """What the set-metric selector reads (pc_set_inputs of the header)."""
    _fields_ = [("n", ctypes.c_int64), ("nown", ctypes.c_int64), ("words", ctypes.c_int32), ("two_holder", ctypes.c_int32),
                ("avg_shared", ctypes.c_double), ("max_nph", ctypes.c_int32), ("max_ngen", ctypes.c_int32),
                ("min_gene_len", ctypes.c_int32), ("max_ent_len", ctypes.c_int32), ("max_tlen", ctypes.c_int64),
                ("max_block_entries", ctypes.c_int64), ("metric", ctypes.c_int32), ("forced", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PcSetShape(ctypes.Structure):
    """Launch shape of a set-metric kernel family (pc_set_shape of the header)."""
    _fields_ = [(name, ctypes.c_int32) for name in ("family", "tile", "super_edge", "grid", "units", "units_per_wg", "chunks", "chunk",
                                                    "batches", "dense", "seg", "runs", "lds", "table", "vals_cap", "reserved")]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


EXPORTS = ["pc_version", "pc_test_hooks", "pc_last_error", "pc_ctx_create", "pc_ctx_destroy", "pc_upload", "pc_set_shard", "pc_set_shard_balanced",
           "pc_shard_pairs", "pc_shard_stride", "pc_fill", "pc_fill_borrow", "pc_fill_dev", "pc_fill_shard_dev", "pc_assemble_dev",
           "pc_align_pairs", "pc_last_align_ms", "pc_round6_probe", "pc_set_tie_rule", "pc_get_tie_rule", "pc_shard_table", "pc_target_costs",
           "pc_plan_dev", "pc_align_slice_dev", "pc_reduce_dev", "pc_upload_sets", "pc_upload_residues", "pc_set_plan_budget", "pc_chunk_plan",
           "pc_variant_width", "pc_task_shape", "pc_ppos_width", "pc_bucket_launch_classes", "pc_last_plan_tasks", "pc_last_set_kernel",
           "pc_set_kernel_choice", "pc_set_launch_shape", "pc_set_max_block_entries", "pc_last_set_launch", "pc_multi_create", "pc_multi_destroy", "pc_multi_devices", "pc_multi_peer_access", "pc_multi_upload",
           "pc_multi_upload_residues", "pc_multi_set_tie_rule", "pc_multi_fill_borrow", "pc_fill_rows", "pc_fill_rows_dev", "pc_fill_edges", "pc_last_edge_times",
           "pc_fill_components", "pc_last_component_times", "pc_fill_groups", "pc_fill_groups_dev", "pc_group_pair_offsets", "pc_group_tiles",
           "pc_fill_nearest", "pc_last_nearest_times", "pc_multi_fill_edges", "pc_multi_fill_components", "pc_multi_fill_nearest",
           "pc_multi_last_stretches", "pc_multi_last_slab_times", "pc_stretch_plan", "pc_fill_tree", "pc_multi_fill_tree", "pc_last_tree_times",
           "pc_last_tree_rounds", "pc_tree_key", "pc_tree_key_parts", "pc_fill_rows_edges", "pc_fill_rows_components", "pc_fill_rows_tree",
           "pc_rows_pass_span", "pc_fill_rows_nearest", "pc_nearest_rows_tile", "pc_fill_between", "pc_multi_fill_between", "pc_last_between_times",
           "pc_between_max_groups", "pc_between_segment", "pc_fill_affinity", "pc_multi_fill_affinity", "pc_last_affinity_times",
           "pc_affinity_block", "pc_affinity_bytes", "pc_affinity_ranges", "pc_hook_slab_values", "pc_hook_rows_values", "pc_fill_rows_affinity",
           "pc_fill_rows_between", "pc_fill_hist", "pc_multi_fill_hist", "pc_fill_rows_hist", "pc_last_hist_times", "pc_hist_bins",
           "pc_hist_table_slots", "pc_hist_probes", "pc_fill_pairs", "pc_fill_pairs_dev", "pc_pair_block",
           "pc_fill_edges_bars", "pc_nearest_of_pairs",
           "pc_fill_joint", "pc_fill_joint_dev", "pc_fill_pairs_joint", "pc_fill_pairs_joint_dev"]
NEEDS_RESIDUES = ("aai", "peq", "aai_ppos")
JOINT_METRICS = ("gcs", "jc", "pocp", "af", "aai", "peq")      # a joint fill's metrics, by bit of its mask (pc_metric 0 ... 5)


def joint_mask(metrics):
    """The C-ABI's metric set of a joint fill: bit ``METRIC_IDS[name]`` for every name of ``metrics``.  Refused here, as the library
    would refuse the mask: an empty set, an unknown name or ``aai_ppos`` (another alignment pass), a name listed twice, and a set with
    neither ``aai`` nor ``peq`` (the set metrics alone share no alignment pass: four millisecond fills)."""
    if isinstance(metrics, str):
        metrics = (metrics,)
    names = list(metrics)
    if not names:
        raise ValueError("joint fill: the metric set is empty")
    mask = 0
    for name in names:
        if name not in JOINT_METRICS:
            raise ValueError(f"joint fill: unknown metric {name!r} (one of {', '.join(JOINT_METRICS)})")
        if mask >> METRIC_IDS[name] & 1:
            raise ValueError(f"joint fill: metric {name!r} is listed twice")
        mask |= 1 << METRIC_IDS[name]
    if not mask & (1 << METRIC_IDS["aai"] | 1 << METRIC_IDS["peq"]):
        raise ValueError("joint fill: the set holds neither aai nor peq; gcs / jc / pocp / af alone are four millisecond fills (fill)")
    return mask
HIST_BINS = 1000001                     # pc_hist_bins(): the millionths in [0, 1]

_lib = None


def load():
    """Load the library (once).  Raises :class:`HipLibraryError` when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(f"{LIB_PATH} not found: build it with `python -m phamclust_amd.build` "
                              f"(there is no CPU fallback)")
    # torch ships its own libamdhip64.so.7; two HIP runtimes in one process cannot both open
    # the GPU.  Importing torch first makes our library bind to the runtime torch uses, so
    # torch tensors, streams and torch.distributed (RCCL) share one device context with it.
    # PHAMCLUST_NO_TORCH=1 (the single-rank CLI sets it) skips that import -- ~1.5 s, a minute or two on a machine that pages torch
    # in for the first time -- for processes that will never import torch: the library then binds to the system's HIP runtime.
    import sys
    if os.environ.get("PHAMCLUST_NO_TORCH") != "1" or "torch" in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as exc:
        raise HipLibraryError(f"cannot load {LIB_PATH}: {exc}") from None
    vp = ctypes.c_void_p
    L.pc_version.restype = ctypes.c_int
    L.pc_test_hooks.restype = ctypes.c_int
    L.pc_last_error.restype = ctypes.c_char_p
    L.pc_ctx_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    L.pc_ctx_destroy.argtypes = [vp]
    L.pc_ctx_destroy.restype = None
    L.pc_upload.argtypes = [vp, ctypes.POINTER(PcPacked)]
    L.pc_upload_sets.argtypes = [vp, ctypes.POINTER(PcPacked)]
    L.pc_upload_residues.argtypes = [vp, ctypes.POINTER(PcPacked)]
    L.pc_set_plan_budget.argtypes = [vp, ctypes.c_int64]
    L.pc_chunk_plan.argtypes = [_u64p, ctypes.c_int, ctypes.c_uint64, _i32p, ctypes.c_int]
    L.pc_variant_width.argtypes = [ctypes.c_int]
    L.pc_task_shape.argtypes = [ctypes.c_int, ctypes.c_int, _i32p]
    L.pc_ppos_width.argtypes = [ctypes.c_int]
    L.pc_bucket_launch_classes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p]
    L.pc_last_plan_tasks.argtypes = [vp, _i32p, ctypes.c_int]
    L.pc_set_shard.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.pc_set_shard_balanced.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.pc_shard_pairs.argtypes = [vp]
    L.pc_shard_pairs.restype = ctypes.c_int64
    L.pc_shard_stride.argtypes = [vp]
    L.pc_shard_stride.restype = ctypes.c_int64
    L.pc_fill.argtypes = [vp, ctypes.c_int, ctypes.c_int, _f64p, ctypes.POINTER(PcStats)]
    L.pc_fill_borrow.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_f64p), ctypes.POINTER(PcStats)]
    L.pc_fill_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.POINTER(PcStats)]
    L.pc_fill_shard_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.POINTER(PcStats)]
    L.pc_assemble_dev.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    L.pc_fill_rows.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _f64p, ctypes.POINTER(PcStats)]
    L.pc_fill_rows_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, vp, vp, ctypes.POINTER(PcStats)]
    L.pc_fill_groups.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, _i64p, ctypes.c_int, _f64p, ctypes.POINTER(PcStats)]
    L.pc_fill_groups_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, _i64p, ctypes.c_int, vp, vp, ctypes.POINTER(PcStats)]
    L.pc_group_pair_offsets.argtypes = [_i64p, ctypes.c_int, _i64p]
    L.pc_group_pair_offsets.restype = ctypes.c_int64
    L.pc_group_tiles.argtypes = [_i64p, ctypes.c_int, _i32p, _i32p, ctypes.c_int64]
    L.pc_group_tiles.restype = ctypes.c_int64
    L.pc_fill_pairs.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, _i32p, ctypes.c_int64, _f64p, ctypes.POINTER(PcStats)]
    L.pc_fill_pairs_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, _i32p, ctypes.c_int64, vp, vp, ctypes.POINTER(PcStats)]
    L.pc_pair_block.restype = ctypes.c_int
    L.pc_fill_joint.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(PcStats)]
    L.pc_fill_joint_dev.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(vp), vp, ctypes.POINTER(PcStats)]
    L.pc_fill_pairs_joint.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, _i32p, _i32p, ctypes.c_int64, ctypes.POINTER(vp), ctypes.POINTER(PcStats)]
    L.pc_fill_pairs_joint_dev.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, _i32p, _i32p, ctypes.c_int64, ctypes.POINTER(vp), vp, ctypes.POINTER(PcStats)]
    L.pc_fill_edges.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                ctypes.POINTER(_f64p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_fill_edges_bars.argtypes = [vp, ctypes.c_int, ctypes.c_int, _f64p, ctypes.c_int64, ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                     ctypes.POINTER(_f64p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_nearest_of_pairs.argtypes = [vp, _i32p, _i32p, _f64p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_i32p), ctypes.POINTER(_f64p),
                                      ctypes.POINTER(_i32p), ctypes.POINTER(ctypes.c_int32)]
    L.pc_last_edge_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_fill_components.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_i32p),
                                     ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_last_component_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_fill_nearest.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_i32p), ctypes.POINTER(_f64p),
                                  ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_last_nearest_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_fill_tree.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_i32p), ctypes.POINTER(_i32p), ctypes.POINTER(_f64p),
                               ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_last_tree_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_last_tree_rounds.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.pc_tree_key.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    L.pc_tree_key.restype = ctypes.c_uint64
    L.pc_tree_key_parts.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.pc_fill_rows_edges.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _i32p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_i32p),
                                     ctypes.POINTER(_i32p), ctypes.POINTER(_f64p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                                     ctypes.POINTER(PcStats)]
    L.pc_fill_rows_components.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, _i32p, ctypes.c_int, _i32p, ctypes.c_int64,
                                          ctypes.POINTER(_i32p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_fill_rows_tree.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int32, ctypes.c_int64,
                                    ctypes.POINTER(_i32p), ctypes.POINTER(_i32p), ctypes.POINTER(_f64p), ctypes.POINTER(ctypes.c_int32),
                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_rows_pass_span.argtypes = [ctypes.c_int]
    L.pc_fill_rows_nearest.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _i32p, _f64p, ctypes.c_int32, ctypes.c_int64,
                                       ctypes.POINTER(_i32p), ctypes.POINTER(_f64p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                       ctypes.POINTER(PcStats)]
    L.pc_nearest_rows_tile.argtypes = []
    L.pc_fill_between.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_i64p), ctypes.POINTER(_i64p),
                                  ctypes.POINTER(_i32p), ctypes.POINTER(_i32p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_last_between_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_between_max_groups.argtypes = []
    L.pc_between_segment.argtypes = []
    L.pc_fill_affinity.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                   ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                   ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                   ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_fill_rows_affinity.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                        ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                        ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                        ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                        ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_fill_rows_between.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _i32p, ctypes.c_int, _i64p, _i64p, _i32p, _i32p, ctypes.c_int64,
                                       ctypes.POINTER(_i64p), ctypes.POINTER(_i64p), ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_fill_hist.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_i64p), ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_fill_rows_hist.argtypes = [vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _i32p, ctypes.c_int, _i64p, ctypes.c_int64, ctypes.POINTER(_i64p),
                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PcStats)]
    L.pc_last_hist_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_hist_bins.argtypes = []
    L.pc_hist_table_slots.argtypes = []
    L.pc_hist_probes.argtypes = []
    L.pc_last_affinity_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_affinity_block.argtypes = []
    L.pc_affinity_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.pc_affinity_bytes.restype = ctypes.c_int64
    L.pc_affinity_ranges.argtypes = [_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int]
    L.pc_hook_slab_values.argtypes = [_f64p, ctypes.c_int64]
    L.pc_hook_rows_values.argtypes = [_f64p, ctypes.c_int32, ctypes.c_int32]
    L.pc_plan_dev.argtypes = [vp, ctypes.c_int, vp, ctypes.POINTER(PcStats)]
    L.pc_align_slice_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.POINTER(PcStats)]
    L.pc_reduce_dev.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    L.pc_align_pairs.argtypes = [vp, _i32p, _i32p, ctypes.c_int64, ctypes.c_int, _i32p, _i32p]
    L.pc_round6_probe.argtypes = [vp, _f64p, _f64p, ctypes.c_int64]
    L.pc_last_align_ms.argtypes = [vp]
    L.pc_last_align_ms.restype = ctypes.c_float
    L.pc_shard_table.argtypes = [vp, _i32p, _i64p]
    L.pc_target_costs.argtypes = [vp, _u64p]
    L.pc_last_set_kernel.argtypes = [vp]
    L.pc_set_kernel_choice.argtypes = [ctypes.POINTER(PcSetInputs)]
    L.pc_set_launch_shape.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, _i32p, ctypes.POINTER(PcSetShape)]
    L.pc_set_max_block_entries.argtypes = [ctypes.POINTER(ctypes.c_uint32), _i32p, ctypes.c_int64]
    L.pc_set_max_block_entries.restype = ctypes.c_int64
    L.pc_last_set_launch.argtypes = [vp, ctypes.POINTER(PcSetInputs), ctypes.POINTER(PcSetShape)]
    L.pc_multi_create.argtypes = [ctypes.POINTER(vp), _i32p, ctypes.c_int]
    L.pc_multi_destroy.argtypes = [vp]
    L.pc_multi_destroy.restype = None
    L.pc_multi_devices.argtypes = [vp]
    L.pc_multi_peer_access.argtypes = [vp, _i32p]
    L.pc_multi_upload.argtypes = [vp, ctypes.POINTER(PcPacked), ctypes.c_int]
    L.pc_multi_upload_residues.argtypes = [vp, ctypes.POINTER(PcPacked)]
    L.pc_multi_set_tie_rule.argtypes = [vp, ctypes.c_int]
    L.pc_multi_fill_borrow.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_f64p), ctypes.POINTER(PcStats),
                                       ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_multi_fill_edges.argtypes = L.pc_fill_edges.argtypes
    L.pc_multi_fill_components.argtypes = L.pc_fill_components.argtypes
    L.pc_multi_fill_nearest.argtypes = L.pc_fill_nearest.argtypes
    L.pc_multi_fill_tree.argtypes = L.pc_fill_tree.argtypes
    L.pc_multi_fill_between.argtypes = L.pc_fill_between.argtypes
    L.pc_multi_fill_affinity.argtypes = L.pc_fill_affinity.argtypes
    L.pc_multi_fill_hist.argtypes = L.pc_fill_hist.argtypes
    L.pc_multi_last_stretches.argtypes = [vp, _i32p]
    L.pc_multi_last_slab_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pc_stretch_plan.argtypes = [_u64p, ctypes.c_int, ctypes.c_int, _i32p]
    L.pc_set_tie_rule.argtypes = [vp, ctypes.c_int]
    L.pc_get_tie_rule.argtypes = [vp]
    _lib = L
    return L


def _ptr(arr, typ):
    return arr.ctypes.data_as(typ)


# -- test hook: the values of the triangular slab walks (libphamclust_hip_hooks.so only) -------------------------------------------
_slab_values = None                     # the array the library holds a pointer to: kept alive here until it is replaced or cleared


def set_slab_values(values):
    """``pc_hook_slab_values``: ``values`` -- float64, C-contiguous, the whole triangle target-major (:func:`triangle_of`) -- stands
    for every slab that ``fill_edges`` / ``_components`` / ``_nearest`` / ``_tree`` / ``_between`` / ``_affinity`` / ``_hist`` of any context of
    this process fills from now on; ``None`` clears it.  The array is referenced, not copied: do not write to it while it is set.  Only
    the test-hooks twin (``PHAMCLUST_NATIVE_VARIANT=hooks``) takes it; the release library refuses, and so does this."""
    global _slab_values
    lib = load()
    if values is None:
        rc = lib.pc_hook_slab_values(None, 0)
    else:
        if not (isinstance(values, np.ndarray) and values.dtype == np.float64 and values.ndim == 1 and values.flags.c_contiguous):
            raise ValueError("set_slab_values: a one-dimensional C-contiguous float64 array, or None")
        rc = lib.pc_hook_slab_values(_ptr(values, _f64p), int(values.shape[0]))
    if rc != 0:
        raise HipLibraryError(f"libphamclust_hip: status {rc}: {lib.pc_last_error().decode()}")
    _slab_values = values


# -- test hook: the values of the rows walk (libphamclust_hip_hooks.so only) --------------------------------------------------------
_rows_values = None                     # the array the library holds a pointer to: kept alive here until it is replaced or cleared


def set_rows_values(values):
    """``pc_hook_rows_values``: ``values`` -- float64, C-contiguous, ``[n_rows, N]``, row k the values of the call's query genome
    ``rows[k]`` -- stands for every slab that ``fill_rows_edges`` / ``_components`` / ``_tree`` / ``_nearest`` / ``_affinity`` / ``_between`` / ``_hist`` of any context of this
    process fills from now on, every element of it: the diagonal ``[k, rows[k]]`` and both copies of a pair of two query genomes are
    the caller's too.  ``None`` clears it.  Independent of :func:`set_slab_values`.  The array is referenced, not copied: do not write
    to it while it is set.  Only the test-hooks twin (``PHAMCLUST_NATIVE_VARIANT=hooks``) takes it; the release library refuses, and
    so does this."""
    global _rows_values
    lib = load()
    if values is None:
        rc = lib.pc_hook_rows_values(None, 0, 0)
    else:
        if not (isinstance(values, np.ndarray) and values.dtype == np.float64 and values.ndim == 2 and values.flags.c_contiguous):
            raise ValueError("set_rows_values: a two-dimensional C-contiguous float64 array, or None")
        rc = lib.pc_hook_rows_values(_ptr(values, _f64p), int(values.shape[0]), int(values.shape[1]))
    if rc != 0:
        raise HipLibraryError(f"libphamclust_hip: status {rc}: {lib.pc_last_error().decode()}")
    _rows_values = values


def triangle_of(square):
    """The triangle the slab walks fill, from a symmetric ``N x N`` array: target-major, element ``t (t - 1) / 2 + s`` the pair
    ``(s, t)``, ``s < t`` -- the strict lower triangle row by row."""
    square = np.asarray(square)
    if square.ndim != 2 or square.shape[0] != square.shape[1]:
        raise ValueError(f"triangle_of: a square array, not {square.shape}")
    t, s = np.tril_indices(square.shape[0], k=-1)
    return np.ascontiguousarray(square[t, s])


def square_of(triangle, n, diagonal=0.0):
    """The symmetric ``n x n`` array of a target-major triangle (:func:`triangle_of`'s inverse), ``diagonal`` on the diagonal."""
    triangle = np.asarray(triangle)
    if triangle.shape != (int(n) * (int(n) - 1) // 2,):
        raise ValueError(f"square_of: {triangle.shape} values for {n} genomes")
    out = np.full((int(n), int(n)), diagonal, dtype=triangle.dtype)
    t, s = np.tril_indices(int(n), k=-1)
    out[t, s] = triangle
    out[s, t] = triangle
    return out


class BorrowedArray(np.lib.mixins.NDArrayOperatorsMixin):
    """Result of ``Context.fill(borrow=True)``: a read-only window on page-locked memory the context owns.  It keeps the
    context alive (so the memory is not freed behind it by garbage collection), and once the loan has ended -- the next fill or
    upload on the context, or its ``close()`` -- every way into the data raises instead of reading recycled memory.

    It is deliberately NOT an ``ndarray`` subclass: numpy hands an ndarray subclass's buffer to ``np.asarray`` /
    ``np.ascontiguousarray`` without asking it (r03's class was one, and those two read a dead loan silently).  Being a foreign
    object, everything numpy does with it starts at ``__array__`` / ``__array_ufunc__`` / ``__array_function__``, and all three
    check the loan.  While the loan lasts, those calls see an ordinary read-only view (zero copy); ``x.copy()`` gives an
    array that owns its memory.  What cannot be guarded is a plain view or pointer taken while the loan was alive and kept."""

    __slots__ = ("_view", "_owner", "_live", "_root", "__weakref__")

    def __init__(self, view, owner, root=None):
        self._view, self._owner, self._live = view, owner, True
        self._root = self if root is None else root         # slices of a loan share its fate through the root object

    def _end_loan(self):
        self._live, self._owner = False, None

    def _check_loan(self):
        if not self._root._live:
            raise HipLibraryError("this array was lent by Context.fill(borrow=True) and the loan has ended (a later fill / "
                                  "upload / close on the context recycled its memory); copy it while it is valid")

    shape = property(lambda self: self._view.shape)
    dtype = property(lambda self: self._view.dtype)
    size = property(lambda self: self._view.size)
    ndim = property(lambda self: self._view.ndim)
    nbytes = property(lambda self: self._view.nbytes)

    def __len__(self):
        return len(self._view)

    def __getitem__(self, item):
        self._check_loan()
        got = self._view[item]
        return BorrowedArray(got, None, self._root) if isinstance(got, np.ndarray) and got.base is not None else got

    def __setitem__(self, item, value):                       # lent memory is the context's: read-only, like the view under it
        raise ValueError("assignment destination is read-only (a borrowed result of Context.fill)")

    def __iter__(self):
        self._check_loan()
        return iter(self._view)

    def __array__(self, dtype=None, copy=None):
        self._check_loan()
        if dtype is not None and np.dtype(dtype) != self._view.dtype:
            return self._view.astype(dtype)
        return self._view.copy() if copy else self._view

    def copy(self, order="C"):
        self._check_loan()
        return np.array(self._view, order=order, copy=True)

    def __getattr__(self, name):                             # .max(), .sum(), .tolist(), .astype() ...: the view's, after the check
        if name.startswith("_"):
            raise AttributeError(name)
        self._check_loan()
        return getattr(self._view, name)

    @staticmethod
    def _plain(x):
        if isinstance(x, BorrowedArray):
            x._check_loan()
            return x._view
        if isinstance(x, (list, tuple)):
            return type(x)(BorrowedArray._plain(y) for y in x)
        if isinstance(x, dict):
            return {k: BorrowedArray._plain(v) for k, v in x.items()}
        return x

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        return getattr(ufunc, method)(*self._plain(inputs), **self._plain(kwargs))

    def __array_function__(self, func, types, args, kwargs):
        return func(*self._plain(args), **self._plain(kwargs))

    def __repr__(self):
        return f"BorrowedArray({'live' if self._root._live else 'loan ended'}, shape={self.shape}, dtype={self.dtype})"


class _SlabFills:
    """``fill_edges`` / ``fill_components`` / ``fill_nearest`` / ``fill_tree`` / ``fill_between`` / ``fill_affinity`` / ``fill_hist`` -- the fills that deliver no dense matrix -- once for :class:`Context`
    and :class:`MultiContext`.  The class supplies ``_SLAB_CALL`` (the prefix of the library's symbols), ``_before_slab_fill(metric)``
    (the residues on demand, earlier loans ended; returns the call's stats object) and ``_slab_stats(kind, stats, **own)`` (the stats
    dict of such a fill)."""

    def _slab_call(self, symbol, metric, *args):
        stats = self._before_slab_fill(metric)
        self._check(getattr(self._lib, symbol)(self._h, METRIC_IDS[metric], *args, stats))
        return stats

    # One decoder per result shape, for the whole form and the rows form alike: the call ``prefix + kind`` with ``args`` (what the call
    # takes between the metric and its output cells), the output cells as arrays or loans, and with ``want_stats`` the stats dict.
    def _fill_edge_arrays(self, kind, prefix, metric, args, want_stats, borrow, symbol=None):
        """``(src, tgt, val)`` of an edge list (``"edges"``: a 64-bit count; ``"tree"``: a 32-bit one, and the round counts);
        ``symbol``: the call, where it is not ``prefix + kind``."""
        ps, pt, pv = _i32p(), _i32p(), _f64p()
        n, nsl = (ctypes.c_int32 if kind == "tree" else ctypes.c_int64)(0), ctypes.c_int32(0)
        stats = self._slab_call(symbol or prefix + kind, metric, *args, ctypes.byref(ps), ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(n), ctypes.byref(nsl))
        out = [self._lend(ptr, (n.value,), borrow) if n.value and ptr else np.empty(0, dtype=dtype)
               for ptr, dtype in ((ps, np.int32), (pt, np.int32), (pv, np.float64))]
        if not want_stats:
            return tuple(out)
        own = self._tree_rounds() if kind == "tree" else {}
        return (*out, self._slab_stats(kind, stats, n_edges=int(n.value), n_slabs=int(nsl.value), **own))

    def _fill_labels(self, prefix, metric, args, want_stats, borrow):
        """``labels`` of a components fill."""
        pl = _i32p()
        nc, ne, nsl = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
        stats = self._slab_call(prefix + "components", metric, *args, ctypes.byref(pl), ctypes.byref(nc), ctypes.byref(ne), ctypes.byref(nsl))
        n = self.n_genomes
        labels = self._lend(pl, (n,), borrow) if n and pl else np.empty(0, dtype=np.int32)
        if not want_stats:
            return labels
        return labels, self._slab_stats("components", stats, n_components=int(nc.value), n_edges=int(ne.value), n_slabs=int(nsl.value))

    def _fill_lists(self, prefix, metric, args, want_stats, borrow):
        """``(nbr, val)`` of a nearest-neighbours fill."""
        pn, pv = _i32p(), _f64p()
        kk, nsl = ctypes.c_int32(0), ctypes.c_int32(0)
        stats = self._slab_call(prefix + "nearest", metric, *args, ctypes.byref(pn), ctypes.byref(pv), ctypes.byref(kk), ctypes.byref(nsl))
        n = self.n_genomes
        if n and kk.value and pn and pv:
            nbr, val = self._lend(pn, (n, kk.value), borrow), self._lend(pv, (n, kk.value), borrow)
        else:
            nbr, val = np.empty((n, 0), dtype=np.int32), np.empty((n, 0), dtype=np.float64)
        if not want_stats:
            return nbr, val
        return nbr, val, self._slab_stats("nearest", stats, k=int(kk.value), n_slabs=int(nsl.value))

    def _fill_table(self, prefix, metric, args, n_groups, want_stats, borrow):
        """``(sum, count, lo, hi)`` of a between-groups fill."""
        ps, pc, pl, ph = _i64p(), _i64p(), _i32p(), _i32p()
        nsl = ctypes.c_int32(0)
        stats = self._slab_call(prefix + "between", metric, *args, ctypes.byref(ps), ctypes.byref(pc), ctypes.byref(pl), ctypes.byref(ph), ctypes.byref(nsl))
        out = tuple(self._lend(ptr, (n_groups, n_groups), borrow) for ptr in (ps, pc, pl, ph))
        if not want_stats:
            return out
        return (*out, self._slab_stats("between", stats, n_groups=int(n_groups), n_slabs=int(nsl.value)))

    def fill_between(self, metric, group, n_groups=None, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """For a partition of the genomes -- ``group[g]`` in ``[0, n_groups)`` is genome g's group; ``n_groups`` defaults to the largest
        label + 1 -- the table of the pair values between every two groups, and within each group on the diagonal, as ``(sum, count,
        lo, hi)``: int64, int64, int32, int32 arrays ``[G, G]``, symmetric, in MILLIONTHS of the whole distance fill's values; with
        ``as_distance=False`` the similarity table, which is that table inverted (``GroupLinkage.inverted``: every millionth's
        complement, what ``SymMatrix.invert`` makes of the distance matrix -- at a decimal tie not what a similarity fill rounds to).  ``lo`` is the single-linkage, ``hi`` the complete-linkage and ``sum / count`` the
        average-linkage value of two groups (``matrix.GroupLinkage`` reads them); integers, so the table is exact whatever the slab
        cut or the number of devices.  An entry no pair fell into reads ``count = 0, sum = 0, lo = 2**31 - 1, hi = -1``.  The dense
        matrix is neither delivered nor (beyond ``slab_bytes`` of HBM at a time; 0 = automatic) held, as by :meth:`fill_edges`.
        ``n_groups`` above ``Context.BETWEEN_MAX_GROUPS`` and a label out of range are refused by the library.  The arrays are copies;
        ``borrow=True`` lends the context's page-locked memory instead, on ``fill(borrow=True)``'s terms.  ``want_stats`` adds the
        fills' summed stats with ``n_groups``, ``n_slabs``, ``ms_reduce`` and ``ms_finish``.

        On a :class:`MultiContext`: the same arrays -- every device accumulates over its stretch of targets, the root adds the
        accumulators (``k_between_merge``) and folds; the stats carry the route's own entries (as for :meth:`fill_edges`) in place of
        the two times."""
        if group is None:
            raise ValueError("fill_between: group is None")
        group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        if group.shape[0] != self.n_genomes:
            raise ValueError(f"fill_between: group holds {group.shape[0]} labels for {self.n_genomes} genomes")
        if n_groups is None:
            n_groups = int(group.max()) + 1 if group.size else 1
        n_groups = int(n_groups)
        pgroup = _ptr(group if group.size else np.zeros(1, dtype=np.int32), _i32p)
        return self._fill_table(self._SLAB_CALL, metric, (int(bool(as_distance)), pgroup, n_groups, int(slab_bytes)), n_groups, want_stats, borrow)

    def _fill_hist(self, prefix, metric, args, want_stats, borrow):
        """``hist`` of a distribution fill: int64 ``[n_classes, HIST_BINS]``."""
        ph = _i64p()
        ncl, npairs, nsl = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
        stats = self._slab_call(prefix + "hist", metric, *args, ctypes.byref(ph), ctypes.byref(ncl), ctypes.byref(npairs), ctypes.byref(nsl))
        hist = self._lend(ph, (int(ncl.value), HIST_BINS), borrow)
        if not want_stats:
            return hist
        return hist, self._slab_stats("hist", stats, n_classes=int(ncl.value), hist_pairs=int(npairs.value), n_slabs=int(nsl.value))

    def _hist_group(self, who, group, n_groups):
        """``(group array or None, its pointer or NULL, n_groups)`` of a distribution fill."""
        if group is None:
            return None, None, 0
        group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        if group.shape[0] != self.n_genomes:
            raise ValueError(f"{who}: group holds {group.shape[0]} labels for {self.n_genomes} genomes")
        if n_groups is None:
            n_groups = int(group.max()) + 1 if group.size else 1
        return group, _ptr(group if group.size else np.zeros(1, dtype=np.int32), _i32p), int(n_groups)

    def fill_hist(self, metric, group=None, n_groups=None, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """The exact histogram of every pair value, without the dense matrix: int64 ``[n_classes, HIST_BINS]``, bin k the pairs whose
        value is k millionths (every delivered value is ``round(x, 6)``: the histogram IS the distribution).  ``group=None``: one
        class.  ``group[g]`` in ``[0, n_groups)`` (``n_groups`` defaults to the largest label + 1; no cap): two classes, row 0 the
        pairs inside a group, row 1 the pairs between two.  The bins sum to ``N (N - 1) / 2``.  ``as_distance=False``: the histogram
        of the inverted matrix, every row reversed (as :meth:`fill_between` inverts; at a decimal tie not a similarity fill's
        values).  ``matrix.PairDistribution`` reads the array: counts within any threshold, quantiles, exact moments.  The dense
        matrix is neither delivered nor (beyond ``slab_bytes`` of HBM at a time; 0 = automatic) held, as by :meth:`fill_edges`.
        The array is a copy; ``borrow=True`` lends the context's page-locked memory instead, on ``fill(borrow=True)``'s terms.
        ``want_stats`` adds the fills' summed stats with ``n_classes``, ``hist_pairs`` (the sum of all bins), ``n_slabs``, ``ms_pass`` and ``ms_finish``.

        On a :class:`MultiContext`: the same array -- every device counts over its stretch of targets, the root adds the shipped
        histograms (``k_hist_merge``) and finishes; the stats carry the route's own entries in place of the two times."""
        group, pgroup, n_groups = self._hist_group("fill_hist", group, n_groups)
        return self._fill_hist(self._SLAB_CALL, metric, (int(bool(as_distance)), pgroup, n_groups, int(slab_bytes)), want_stats, borrow)

    @staticmethod
    def hist_table_slots():
        """Slots of the LDS table a workgroup of the distribution pass counts its chunk in (``pc_hist_table_slots``; no GPU)."""
        return int(load().pc_hist_table_slots())

    @staticmethod
    def hist_probes():
        """Slots an insert into that table tries before it adds to the global bin (``pc_hist_probes``; no GPU)."""
        return int(load().pc_hist_probes())

    @staticmethod
    def hist_slot(key):
        """The first slot of ``key = cls << 20 | micro`` in that table: the top bits of ``key * 2654435761 mod 2**32`` (the hash the
        C header documents; host arithmetic for the tests that build probe runs)."""
        slots = _SlabFills.hist_table_slots()
        return ((int(key) * 2654435761) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))

    def fill_affinity(self, metric, group, n_groups=None, as_distance=True, slab_bytes=0, want_table=False, want_stats=False, borrow=False):
        """How every genome relates to every group of a partition (``group`` / ``n_groups`` as :meth:`fill_between` takes them), in
        MILLIONTHS of the whole distance fill's values and without the dense matrix.  Returns a dict of arrays: ``own_sum`` (int64),
        ``own_lo``, ``own_hi`` (int32) ``[N]`` -- sum, minimum and maximum of a genome's values to the OTHER members of its own group;
        ``near_group`` (int32 ``[3, N]``) -- the other non-empty group nearest by 0: smallest mean, 1: smallest minimum, 2: smallest
        maximum (ties to the smaller index, -1: none) -- with ``near_sum`` (int64), ``near_lo``, ``near_hi`` (int32) ``[N]``, the value
        that made it nearest; and ``table``: None, or with ``want_table=True`` the whole ``(sum, lo, hi)`` of ``[N, G]`` arrays.  The
        count of entry ``[g, b]`` is ``size[b] - (group[g] == b)``; an entry no pair falls into reads ``0, 2**31 - 1, -1``.  The N x G
        table stays on the device (:meth:`affinity_bytes`; refused above half of the free HBM); only the O(N) arrays cross PCIe unless
        the table is asked for.  ``as_distance=False``: the statement of the inverted matrix -- the same nearest groups, every value
        complemented (``matrix.GroupAffinity.inverted``).  Integers, so the result is exact whatever the slab cut or the number of
        devices.  ``borrow`` as for :meth:`fill_between`; ``want_stats`` adds ``stats`` to the dict: the fills' summed stats with
        ``n_groups``, ``n_slabs``, ``ms_rows``, ``ms_cols`` and ``ms_finish`` (a :class:`MultiContext`: the route's own entries)."""
        if group is None:
            raise ValueError("fill_affinity: group is None")
        group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        if group.shape[0] != self.n_genomes:
            raise ValueError(f"fill_affinity: group holds {group.shape[0]} labels for {self.n_genomes} genomes")
        if n_groups is None:
            n_groups = int(group.max()) + 1 if group.size else 1
        n_groups, n = int(n_groups), self.n_genomes
        pgroup = _ptr(group if group.size else np.zeros(1, dtype=np.int32), _i32p)
        cells = [t() for t in (_i64p, _i32p, _i32p, _i32p, _i64p, _i32p, _i32p, _i64p, _i32p, _i32p)]
        nsl = ctypes.c_int32(0)
        stats = self._slab_call(self._SLAB_CALL + "affinity", metric, int(bool(as_distance)), pgroup, n_groups, int(bool(want_table)), int(slab_bytes),
                                *(ctypes.byref(c) for c in cells), ctypes.byref(nsl))
        names = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")
        dtypes = (np.int64, np.int32, np.int32, np.int32, np.int64, np.int32, np.int32)
        out = {}
        for name, cell, dtype in zip(names, cells, dtypes):
            shape = (3, n) if name == "near_group" else (n,)
            out[name] = self._lend(cell, shape, borrow) if n and cell else np.empty(shape, dtype=dtype)
        out["table"] = None
        if want_table:
            out["table"] = tuple(self._lend(cell, (n, n_groups), borrow) if n and cell else np.empty((n, n_groups), dtype=dtype)
                                 for cell, dtype in zip(cells[7:], (np.int64, np.int32, np.int32)))
        if want_stats:
            out["stats"] = self._slab_stats("affinity", stats, n_groups=n_groups, n_slabs=int(nsl.value))
        return out

    @staticmethod
    def affinity_block():
        """Consecutive sources one wave of the affinity fill's column pass takes (``pc_affinity_block``; host arithmetic, no GPU)."""
        return int(load().pc_affinity_block())

    @staticmethod
    def affinity_bytes(n, n_groups):
        """Bytes of the table an affinity fill of ``n`` genomes in ``n_groups`` groups keeps on the device (``pc_affinity_bytes``: 16 per
        entry and an 8-byte counter; host arithmetic, no GPU)."""
        b = int(load().pc_affinity_bytes(int(n), int(n_groups)))
        if b < 0:
            raise ValueError(f"affinity_bytes: {n} genomes x {n_groups} groups")
        return b

    @staticmethod
    def affinity_ranges(goff, n, want):
        """The group ranges of the affinity fill's column pass as host arithmetic (``pc_affinity_ranges``; no GPU): range starts +
        [G] for ``goff`` (int32 ``[G + 1]``, each group's run among the genomes sorted by group) of ``n`` genomes and about ``want``
        ranges -- a fill asks for ``ceil(16 * CUs / ceil(n / affinity_block()))``."""
        goff = np.ascontiguousarray(goff, dtype=np.int32).reshape(-1)
        bounds = np.zeros(goff.shape[0] + 1, dtype=np.int32)
        lib = load()
        r = lib.pc_affinity_ranges(_ptr(goff, _i32p), int(goff.shape[0]) - 1, int(n), int(want), _ptr(bounds, _i32p), int(bounds.shape[0]))
        if r < 0:
            raise ValueError(lib.pc_last_error().decode())
        return bounds[:r + 1].copy()

    def fill_edges(self, metric, threshold, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """The pairs (s, t), s < t, whose value passes ``threshold`` -- ``d <= threshold`` for a distance fill, ``sim >= threshold``
        for a similarity fill -- as ``(src, tgt, val)``: int32, int32, float64 arrays sorted by ``t``, then ``s``; the values are
        the whole fill's.  The dense matrix is neither delivered nor (beyond ``slab_bytes`` of HBM at a time; 0 = automatic) held.
        The arrays are copies; ``borrow=True`` lends the context's page-locked memory instead, on ``fill(borrow=True)``'s terms.
        ``want_stats`` adds the fills' summed stats with ``n_edges``, ``n_slabs``, ``ms_compact`` and ``ms_d2h``.

        On a :class:`MultiContext`: the same arrays, element for element, whatever the number of devices -- each walks one
        contiguous stretch of targets, and the lists are laid end to end in the root's page-locked memory.  The stats are summed
        over the devices and carry the route's own entries (``per_device``, ``stretches``, ``ms_exchange``, ``ms_merge``,
        ``n_devices``, ``peer_access``) in place of the two times."""
        return self._fill_edge_arrays("edges", self._SLAB_CALL, metric, (int(bool(as_distance)), float(threshold), int(slab_bytes)), want_stats, borrow)

    def fill_components(self, metric, threshold, as_distance=True, strict=True, slab_bytes=0, want_stats=False, borrow=False):
        """The connected components of the graph whose edges are the pairs that pass ``threshold`` -- ``d < threshold`` for a
        distance fill (``d <= threshold`` with ``strict=False``), ``sim > threshold`` (``>=``) for a similarity fill -- as
        ``labels``: int32[N], ``labels[g]`` = the smallest genome index of g's component.  On distances with ``strict`` these are the
        single-linkage clusters at ``eps = threshold``.  Neither the dense matrix nor an edge list is delivered; the matrix is held
        in HBM ``slab_bytes`` at a time (0 = automatic), as by :meth:`fill_edges`.  The array is a copy; ``borrow=True`` lends the
        context's page-locked memory instead, on ``fill(borrow=True)``'s terms.  ``want_stats`` adds the fills' summed stats with
        ``n_components``, ``n_edges`` (pairs that passed), ``n_slabs``, ``ms_union`` and ``ms_labels``.

        On a :class:`MultiContext`: the same canonical ``labels`` -- every device builds the forest of its stretch of targets, the
        root unites them (``k_cc_merge``) and labels; ``n_edges`` counts over all devices, and the stats carry the route's own
        entries (as for :meth:`fill_edges`) in place of the two times."""
        return self._fill_labels(self._SLAB_CALL, metric, (int(bool(as_distance)), float(threshold), int(bool(strict)), int(slab_bytes)), want_stats, borrow)

    def fill_nearest(self, metric, k, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """Each genome's ``kk = min(k, N - 1)`` nearest neighbours as ``(nbr, val)``: int32[N, kk] genome indices and float64[N, kk]
        values, row g listing the genomes h != g best first -- the smallest distance (``as_distance``), else the largest
        similarity -- and equal values in index order: ``SymMatrix.nearest_neighbors(g, threshold)`` with the threshold wide
        open, cut after kk.  The values are the whole fill's.  The dense matrix is neither delivered nor (beyond ``slab_bytes`` of
        HBM at a time; 0 = automatic) held, as by :meth:`fill_edges`.  ``k`` above ``Context.NEAREST_MAX_K`` is refused by the
        library.  The arrays are copies; ``borrow=True`` lends the context's page-locked memory instead, on ``fill(borrow=True)``'s
        terms.  ``want_stats`` adds the fills' summed stats with ``k`` (= kk), ``n_slabs``, ``ms_select`` and ``ms_finish``.

        On a :class:`MultiContext`: the same ``(nbr, val)`` -- the k smallest of one total order, so the lists the devices build
        over their stretches of targets merge by that order on the root (``k_nn_merge``); the stats carry the route's own entries
        (as for :meth:`fill_edges`) in place of the two times."""
        return self._fill_lists(self._SLAB_CALL, metric, (int(bool(as_distance)), int(k), int(slab_bytes)), want_stats, borrow)

    def fill_tree(self, metric, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """The single-linkage dendrogram as the ``N - 1`` edges ``(src, tgt, val)`` -- int32, int32, float64, ``src < tgt`` -- of the
        minimum spanning tree under one total order on the pairs: the better value first (the smallest distance with ``as_distance``,
        else the largest similarity), then the smaller target, then the smaller source; delivered ascending in that order, which is
        the merge order of single linkage.  It is the tree Kruskal's algorithm accepts in that order
        (``matrix.SingleLinkageTree.from_dense`` states it on the host), canonical whatever the slab cut or the number of devices;
        the values are the whole fill's.  From it the clusters at any threshold or for any cluster count, the linkage matrix and the
        leaf order follow on the host.  The dense matrix is neither delivered nor (beyond ``slab_bytes`` of HBM at a time;
        0 = automatic) held, as by :meth:`fill_edges`.  The arrays are copies; ``borrow=True`` lends the context's page-locked memory
        instead, on ``fill(borrow=True)``'s terms.  ``want_stats`` adds the fills' summed stats with ``n_edges``, ``n_slabs``,
        ``ms_rounds``, ``ms_finish``, ``live_rounds`` and ``launched_rounds``.

        On a :class:`MultiContext`: the same arrays -- every device builds the forest of its stretch of targets, the root merges
        the forests by rounds over the lists alone; the stats carry the route's own entries (as for :meth:`fill_edges`) in place of
        the two times."""
        return self._fill_edge_arrays("tree", self._SLAB_CALL, metric, (int(bool(as_distance)), int(slab_bytes)), want_stats, borrow)


class Context(_SlabFills):
    """One GPU.  ``upload`` once, then ``fill`` any of the six metrics."""

    def __init__(self, device_id=0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self._packed = None
        self.device_id = int(device_id)
        self._check(self._lib.pc_ctx_create(ctypes.byref(self._h), int(device_id)))

    def _check(self, rc):
        if rc != 0:
            raise HipLibraryError(f"libphamclust_hip: status {rc}: {self._lib.pc_last_error().decode()}")

    def close(self):
        self._invalidate_loans()
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.pc_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data ------------------------------------------------------------------
    @staticmethod
    def _struct(packed):
        return PcPacked(packed.n_genomes, packed.n_phams, packed.words_per_row, 0,
                        _ptr(packed.bitmap, _u64p), _ptr(packed.nph, _i32p), _ptr(packed.ngen, _i32p),
                        _ptr(packed.tlen, _i64p), _ptr(packed.gene_off, _i64p), _ptr(packed.gene_pham, _i32p),
                        _ptr(packed.seq_off, _i64p), _ptr(packed.residues, _u8p))

    def upload(self, packed, residues=True):
        """Genomes to HBM.  ``residues=False`` uploads only what gcs / jc / pocp / af read (pham sets, gene counts,
        translation lengths: metrics.py:26-157) -- about a tenth of the time; the residues follow by themselves the first
        time an aai / peq fill (or ``align_pairs``) asks for them, from the packed object this context keeps alive."""
        packed.validate()
        s = self._struct(packed)
        self._invalidate_loans()
        self._check((self._lib.pc_upload if residues else self._lib.pc_upload_sets)(self._h, ctypes.byref(s)))
        self._packed = packed
        self._residues = bool(residues)
        self._shard = (0, 1, False)               # pc_upload resets the shard to "everything"
        return self

    def ensure_residues(self):
        if not getattr(self, "_residues", False):
            if self._packed is None:
                raise HipLibraryError("no genomes uploaded")
            s = self._struct(self._packed)
            self._check(self._lib.pc_upload_residues(self._h, ctypes.byref(s)))
            self._residues = True

    def set_plan_budget(self, n_bytes):
        """HBM one chunk of an aai / peq fill's plan may take (0 = automatic); fills above it run in chunks, same values."""
        self._check(self._lib.pc_set_plan_budget(self._h, int(n_bytes)))

    # a borrowed result (fill(borrow=True)) is a view of pinned memory the CONTEXT owns and recycles: every array lent out
    # is remembered weakly and told when its loan ends (BorrowedArray)
    def _invalidate_loans(self):
        for ref in getattr(self, "_loans", []):
            arr = ref()
            if arr is not None:
                arr._end_loan()
        self._loans = []

    def _lend(self, ptr, shape, borrow=True):
        """``shape`` elements at ``ptr``, the context's page-locked memory: lent as a read-only view that is told when its loan
        ends (``borrow``), or copied."""
        view = np.ctypeslib.as_array(ptr, shape=shape)
        if not borrow:
            return view.copy()
        view.flags.writeable = False
        out = BorrowedArray(view, self)
        self._loans.append(weakref.ref(out))
        return out

    @property
    def n_genomes(self):
        return self._packed.n_genomes

    @property
    def n_pairs(self):
        return self._packed.n_pairs

    def set_shard(self, rank, world, balanced=False):
        """Static shard of the pair list; ``balanced`` deals target genomes by measured alignment work instead of
        boustrophedon-wise (same on every rank of a job)."""
        key = (int(rank), int(world), bool(balanced))
        if getattr(self, "_shard", None) != key:
            call = self._lib.pc_set_shard_balanced if balanced else self._lib.pc_set_shard
            self._check(call(self._h, int(rank), int(world)))
            self._shard = key

    def shard_table(self):
        """(t_rank[N], t_lbase[N]) of the deal in force: pair (s, t) is element t_lbase[t] + s of rank t_rank[t]'s shard."""
        t_rank = np.zeros(self.n_genomes, dtype=np.int32)
        t_lbase = np.zeros(self.n_genomes, dtype=np.int64)
        self._check(self._lib.pc_shard_table(self._h, _ptr(t_rank, _i32p), _ptr(t_lbase, _i64p)))
        return t_rank, t_lbase

    def target_costs(self):
        """DP cells behind every target genome (available once a cost-balanced deal has been computed)."""
        cost = np.zeros(self.n_genomes, dtype=np.uint64)
        self._check(self._lib.pc_target_costs(self._h, _ptr(cost, _u64p)))
        return cost

    def shard_pairs(self):
        return int(self._lib.pc_shard_pairs(self._h))

    def shard_stride(self):
        return int(self._lib.pc_shard_stride(self._h))

    # -- fills -------------------------------------------------------------------
    def fill(self, metric, as_distance=True, want_stats=False, borrow=False):
        """Whole matrix -> host condensed f64 vector (scipy order).  ``borrow=True`` returns a READ-ONLY view of page-locked
        memory the context owns (no pageable staging: the D2H copy runs at PCIe speed); the view is only good until the
        next fill or upload on this context -- copy it, or consume it at once as matrix_de_novo does."""
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        self._invalidate_loans()
        if borrow:
            ptr = _f64p()
            self._check(self._lib.pc_fill_borrow(self._h, METRIC_IDS[metric], int(bool(as_distance)), ctypes.byref(ptr), ctypes.byref(stats)))
            out = self._lend(ptr, (max(self.n_pairs, 1),))[:self.n_pairs]
            return (out, stats.as_dict()) if want_stats else out
        out = np.empty(max(self.n_pairs, 0), dtype=np.float64)
        buf = out if out.size else np.zeros(1)
        self._check(self._lib.pc_fill(self._h, METRIC_IDS[metric], int(bool(as_distance)), _ptr(buf, _f64p),
                                      ctypes.byref(stats)))
        return (out, stats.as_dict()) if want_stats else out

    def fill_rows(self, metric, rows, as_distance=True, want_stats=False):
        """The query genomes ``rows`` (distinct indices, strictly ascending) against every other genome -> an ``(M, N)`` float64
        array: ``out[k, g]`` is the whole fill's value of the pair {rows[k], g}, ``out[k, rows[k]]`` the diagonal
        (``1.0 - as_distance``).  New genomes against a filled matrix: what ``matrix.matrix_extend`` calls."""
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        out = np.empty((rows.shape[0], self.n_genomes), dtype=np.float64)
        buf = out if out.size else np.zeros(1)
        self._check(self._lib.pc_fill_rows(self._h, METRIC_IDS[metric], int(bool(as_distance)), _ptr(rows, _i32p), int(rows.shape[0]),
                                           _ptr(buf, _f64p), ctypes.byref(stats)))
        return (out, stats.as_dict()) if want_stats else out

    @staticmethod
    def _group_arrays(groups):
        """``groups`` (sequences of genome indices) as the C-ABI's ``members`` / ``group_off`` arrays."""
        groups = [np.ascontiguousarray(g, dtype=np.int32).reshape(-1) for g in groups]
        off = np.zeros(len(groups) + 1, dtype=np.int64)
        if groups:
            np.cumsum([g.shape[0] for g in groups], out=off[1:])
        members = np.concatenate(groups) if groups else np.empty(0, dtype=np.int32)
        return np.ascontiguousarray(members, dtype=np.int32), off

    @staticmethod
    def group_pair_offsets(group_off):
        """``pair_off[G + 1]`` of a groups fill: where each group's condensed triangle starts; the last entry is L (host arithmetic)."""
        group_off = np.ascontiguousarray(group_off, dtype=np.int64)
        pair_off = np.zeros(group_off.shape[0], dtype=np.int64)
        total = load().pc_group_pair_offsets(_ptr(group_off, _i64p), int(group_off.shape[0]) - 1, _ptr(pair_off, _i64p))
        if total < 0:
            raise ValueError(load().pc_last_error().decode())
        return pair_off

    @staticmethod
    def group_tiles(group_off):
        """The live 32 x 32 tiles ``(row block, column block)`` of a groups fill as an ``(T, 2)`` int32 array, sorted (host arithmetic)."""
        group_off = np.ascontiguousarray(group_off, dtype=np.int64)
        lib, n = load(), int(group_off.shape[0]) - 1
        count = lib.pc_group_tiles(_ptr(group_off, _i64p), n, None, None, 0)
        if count < 0:
            raise ValueError(lib.pc_last_error().decode())
        tiles = np.zeros((2, max(int(count), 1)), dtype=np.int32)
        lib.pc_group_tiles(_ptr(group_off, _i64p), n, _ptr(tiles[0], _i32p), _ptr(tiles[1], _i32p), int(count))
        return np.ascontiguousarray(tiles[:, :int(count)].T)

    def fill_groups(self, metric, groups, as_distance=True, want_stats=False):
        """Every within-group pair of ``groups`` -- sequences of genome indices, each strictly ascending; groups may share genomes
        -- in one call: a list of condensed float64 arrays, one per group (scipy order: what ``SymMatrix.from_condensed`` takes; a
        group of fewer than two members gives an empty array).  Values are the whole fill's, each pair in its orientation."""
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        members, off = self._group_arrays(groups)
        pair_off = self.group_pair_offsets(off)
        out = np.empty(int(pair_off[-1]), dtype=np.float64)
        buf = out if out.size else np.zeros(1)
        self._check(self._lib.pc_fill_groups(self._h, METRIC_IDS[metric], int(bool(as_distance)), _ptr(members if members.size else np.zeros(1, np.int32), _i32p),
                                             _ptr(off, _i64p), len(off) - 1, _ptr(buf, _f64p), ctypes.byref(stats)))
        parts = [out[pair_off[k]:pair_off[k + 1]] for k in range(len(off) - 1)]
        return (parts, stats.as_dict()) if want_stats else parts

    def fill_groups_dev(self, metric, as_distance, groups, out_ptr, stream=None, want_stats=True):
        """The same, left in HBM at ``out_ptr`` as one float64 vector: the groups' condensed triangles end to end
        (:meth:`group_pair_offsets` of the groups' sizes gives the cuts)."""
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        members, off = self._group_arrays(groups)
        self._check(self._lib.pc_fill_groups_dev(self._h, METRIC_IDS[metric], int(bool(as_distance)), _ptr(members if members.size else np.zeros(1, np.int32), _i32p),
                                                 _ptr(off, _i64p), len(off) - 1, ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0),
                                                 ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    @staticmethod
    def _pair_arrays(src, tgt):
        """``src`` / ``tgt`` (genome indices) as the C-ABI's two int32 arrays of one length."""
        src, tgt = np.asarray(src).reshape(-1), np.asarray(tgt).reshape(-1)
        if src.shape[0] != tgt.shape[0]:
            raise ValueError(f"fill_pairs: {src.shape[0]} sources and {tgt.shape[0]} targets")
        for name, arr in (("src", src), ("tgt", tgt)):                 # before the cast: an index beyond 32 bits must not wrap into range
            if arr.size and (arr.dtype.kind not in "iu" or int(arr.min()) < -2 ** 31 or int(arr.max()) >= 2 ** 31):
                raise ValueError(f"fill_pairs: {name} must hold integer genome indices that fit 32 bits")
        return np.ascontiguousarray(src, dtype=np.int32), np.ascontiguousarray(tgt, dtype=np.int32)

    def fill_pairs(self, metric, src, tgt, as_distance=True, want_stats=False):
        """The pairs ``(src[k], tgt[k])`` in one call -> a float64 array in the caller's order: ``out[k]`` is the reference's
        ``METRICS[metric](genomes[src[k]], genomes[tgt[k]])``, ORIENTED as written (with ``src[k] < tgt[k]`` the whole fill's cell;
        reversed, under aai / peq, the other orientation), ``src[k] == tgt[k]`` the diagonal.  A pair may be listed any number of times."""
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        src, tgt = self._pair_arrays(src, tgt)
        out = np.empty(src.shape[0], dtype=np.float64)
        one = np.zeros(1, np.int32)
        self._check(self._lib.pc_fill_pairs(self._h, METRIC_IDS[metric], int(bool(as_distance)), _ptr(src if src.size else one, _i32p),
                                            _ptr(tgt if tgt.size else one, _i32p), int(src.shape[0]), _ptr(out if out.size else np.zeros(1), _f64p),
                                            ctypes.byref(stats)))
        return (out, stats.as_dict()) if want_stats else out

    def fill_pairs_dev(self, metric, as_distance, src, tgt, out_ptr, stream=None, want_stats=True):
        """The same, left in HBM at ``out_ptr`` as one float64 vector in the caller's order (``src`` / ``tgt`` are host arrays)."""
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        src, tgt = self._pair_arrays(src, tgt)
        one = np.zeros(1, np.int32)
        self._check(self._lib.pc_fill_pairs_dev(self._h, METRIC_IDS[metric], int(bool(as_distance)), _ptr(src if src.size else one, _i32p),
                                                _ptr(tgt if tgt.size else one, _i32p), int(src.shape[0]), ctypes.c_void_p(out_ptr),
                                                ctypes.c_void_p(stream or 0), ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    # -- joint fills: several metrics of every pair off one plan and one alignment pass ---------------------------------------------
    @staticmethod
    def _joint_pointers(mask, pointer_of):
        """The C-ABI's ``out[6]``: ``pointer_of(name)`` for every metric of the mask, NULL elsewhere."""
        out = (ctypes.c_void_p * 6)()
        for m, name in enumerate(JOINT_METRICS):
            if mask >> m & 1:
                out[m] = pointer_of(name)
        return out

    def _joint_host(self, mask, n):
        arrays = {name: np.empty(n, dtype=np.float64) for m, name in enumerate(JOINT_METRICS) if mask >> m & 1}
        spare = np.zeros(1)                                            # (an empty array still hands the library a pointer)
        return arrays, self._joint_pointers(mask, lambda name: (arrays[name] if n else spare).ctypes.data)

    def fill_joint(self, metrics, as_distance=True, want_stats=False):
        """Several metrics of the whole matrix off ONE plan and ONE alignment pass -> ``{name: condensed f64 vector}``, every array what
        :meth:`fill` of that metric returns, bit for bit.  ``metrics``: names among gcs, jc, pocp, af, aai, peq, at least one of aai /
        peq among them (:func:`joint_mask`).  The stats are the peq fill's."""
        mask = joint_mask(metrics)
        stats = PcStats()
        self.ensure_residues()
        self._invalidate_loans()
        arrays, out = self._joint_host(mask, max(self.n_pairs, 0))
        self._check(self._lib.pc_fill_joint(self._h, mask, int(bool(as_distance)), out, ctypes.byref(stats)))
        return (arrays, stats.as_dict()) if want_stats else arrays

    def fill_joint_dev(self, metrics, as_distance, out_ptrs, stream=None, want_stats=True):
        """The same, left in HBM: ``out_ptrs`` maps every metric name of the set to the device address of its condensed vector."""
        mask = joint_mask(metrics)
        stats = PcStats()
        self.ensure_residues()
        out = self._joint_pointers(mask, lambda name: int(out_ptrs[name]))
        self._check(self._lib.pc_fill_joint_dev(self._h, mask, int(bool(as_distance)), out, ctypes.c_void_p(stream or 0),
                                                ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    def fill_pairs_joint(self, metrics, src, tgt, as_distance=True, want_stats=False):
        """Several metrics of the pairs ``(src[k], tgt[k])`` off one plan and one alignment pass -> ``{name: f64[L]}`` in the caller's
        order, every array what :meth:`fill_pairs` of that metric returns, bit for bit (oriented as written; repeats allowed;
        ``src[k] == tgt[k]`` the diagonal in every array)."""
        mask = joint_mask(metrics)
        stats = PcStats()
        self.ensure_residues()
        src, tgt = self._pair_arrays(src, tgt)
        arrays, out = self._joint_host(mask, int(src.shape[0]))
        one = np.zeros(1, np.int32)
        self._check(self._lib.pc_fill_pairs_joint(self._h, mask, int(bool(as_distance)), _ptr(src if src.size else one, _i32p),
                                                  _ptr(tgt if tgt.size else one, _i32p), int(src.shape[0]), out, ctypes.byref(stats)))
        return (arrays, stats.as_dict()) if want_stats else arrays

    def fill_pairs_joint_dev(self, metrics, as_distance, src, tgt, out_ptrs, stream=None, want_stats=True):
        """The same, left in HBM: ``out_ptrs`` maps every metric name of the set to the device address of its ``f64[L]``."""
        mask = joint_mask(metrics)
        stats = PcStats()
        self.ensure_residues()
        src, tgt = self._pair_arrays(src, tgt)
        out = self._joint_pointers(mask, lambda name: int(out_ptrs[name]))
        one = np.zeros(1, np.int32)
        self._check(self._lib.pc_fill_pairs_joint_dev(self._h, mask, int(bool(as_distance)), _ptr(src if src.size else one, _i32p),
                                                      _ptr(tgt if tgt.size else one, _i32p), int(src.shape[0]), out,
                                                      ctypes.c_void_p(stream or 0), ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    def fill_edges_bars(self, metric, bars, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """:meth:`fill_edges` with a bar per genome in the threshold's place: the pairs (s, t), s < t, whose value passes ``bars[s]``
        OR ``bars[t]`` -- ``d <= bar`` for a distance fill, ``sim >= bar`` for a similarity fill -- as ``(src, tgt, val)`` in
        :meth:`fill_edges`' order, with its values, loan rule and stats.  ``bars``: N floats; ``+-inf`` is legal, NaN is refused by the
        library, naming the genome.  With all bars equal it is ``fill_edges`` at that threshold, element for element.  One GPU."""
        bars = np.ascontiguousarray(np.asarray(bars, dtype=np.float64).reshape(-1))
        if bars.shape[0] != self.n_genomes:
            raise ValueError(f"fill_edges_bars: {bars.shape[0]} bars for {self.n_genomes} genomes")
        return self._fill_edge_arrays("edges", "pc_fill_", metric, (int(bool(as_distance)), _ptr(bars if bars.size else np.zeros(1), _f64p), int(slab_bytes)),
                                      want_stats, borrow, symbol="pc_fill_edges_bars")

    NEAREST_PAIRS_MAX = 2 ** 30           # pairs one nearest_of_pairs call takes (2 entries each, sorted with 32-bit values)

    def nearest_of_pairs(self, src, tgt, val, k, as_distance=True, borrow=False):
        """K-nearest lists of a pair list: ``(nbr, val, count)`` -- int32[N, kk], float64[N, kk], int32[N], ``kk = min(k, N - 1)``.
        Every listed pair ``{src[e], tgt[e]}`` with value ``val[e]`` is a candidate of both its ends; ``count[g]`` is how many touch
        genome g, and row g lists the best ``min(kk, count[g])`` of them in :meth:`fill_nearest`'s total order (better value first,
        then the smaller index), the slots behind them ``-1`` / NaN.  The list may come in any order; a diagonal entry is refused,
        and the caller promises that no pair is listed twice.  ``SparseEdges.nearest`` states the same on the host.  The context
        gives N only; nothing is filled.  The arrays are copies; ``borrow=True`` lends the context's page-locked memory."""
        src, tgt = self._pair_arrays(src, tgt)
        val = np.ascontiguousarray(np.asarray(val, dtype=np.float64).reshape(-1))
        if val.shape[0] != src.shape[0]:
            raise ValueError(f"nearest_of_pairs: {src.shape[0]} pairs and {val.shape[0]} values")
        self._invalidate_loans()
        pn, pv, pc = _i32p(), _f64p(), _i32p()
        kk = ctypes.c_int32(0)
        one = np.zeros(1, np.int32)
        self._check(self._lib.pc_nearest_of_pairs(self._h, _ptr(src if src.size else one, _i32p), _ptr(tgt if tgt.size else one, _i32p),
                                                  _ptr(val if val.size else np.zeros(1), _f64p), int(src.shape[0]), int(bool(as_distance)), int(k),
                                                  ctypes.byref(pn), ctypes.byref(pv), ctypes.byref(pc), ctypes.byref(kk)))
        n = self.n_genomes
        count = self._lend(pc, (n,), borrow) if n and pc else np.zeros(n, dtype=np.int32)
        if n and kk.value and pn and pv:
            return self._lend(pn, (n, kk.value), borrow), self._lend(pv, (n, kk.value), borrow), count
        return np.empty((n, 0), dtype=np.int32), np.empty((n, 0), dtype=np.float64), count

    EDGE_MAX_PAIRS = 2 ** 31 - 1          # pairs one slab of an edge-list fill may hold (u32 counts and offsets on the device)

    @staticmethod
    def edge_slabs(n, slab_bytes):
        """The ranges of target genomes an edge-list fill of ``n`` genomes walks under ``slab_bytes`` (> 0) of slab: range starts
        + [n] (host arithmetic, no GPU).  It is :meth:`chunk_plan` over ``count[t] = t`` -- target t has t pairs (s, t), s < t --
        with ``slab_bytes // 8`` pairs per range, clamped to 2^31-1; a target above that gets a range of its own."""
        if int(slab_bytes) <= 0:
            raise ValueError("edge_slabs: slab_bytes must be positive (0 = automatic is decided on the device, by the free HBM)")
        return Context.chunk_plan(np.arange(int(n), dtype=np.uint64), min(max(int(slab_bytes) // 8, 1), Context.EDGE_MAX_PAIRS))

    # -- fill_edges / fill_components / fill_nearest / fill_tree (_SlabFills): what this class supplies ----------------------------------
    _SLAB_CALL = "pc_fill_"
    _SLAB_TIMES = {"edges": ("pc_last_edge_times", "ms_compact", "ms_d2h"), "components": ("pc_last_component_times", "ms_union", "ms_labels"),
                   "nearest": ("pc_last_nearest_times", "ms_select", "ms_finish"), "tree": ("pc_last_tree_times", "ms_rounds", "ms_finish"), "between": ("pc_last_between_times", "ms_reduce", "ms_finish"), "hist": ("pc_last_hist_times", "ms_pass", "ms_finish"),
                   "affinity": ("pc_last_affinity_times", "ms_rows", "ms_cols", "ms_finish")}
    TREE_MAX_GENOMES = 1 << 22            # PC_TREE_MAX_GENOMES: a genome index takes 22 bits of a tree key
    BETWEEN_MAX_GROUPS = 2048             # PC_BETWEEN_MAX_GROUPS: the pass keeps one entry per group in LDS

    @staticmethod
    def between_segment():
        """Elements of a slab row one workgroup of the between-groups pass takes (``pc_between_segment``; host arithmetic, no GPU): what
        a test of the pass's segment seams sizes its inputs by."""
        return int(load().pc_between_segment())

    def _tree_rounds(self):
        """``live_rounds`` / ``launched_rounds`` of the last tree fill (``pc_last_tree_rounds``)."""
        live, launched = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.pc_last_tree_rounds(self._h, ctypes.byref(live), ctypes.byref(launched)))
        return dict(live_rounds=int(live.value), launched_rounds=int(launched.value))

    @staticmethod
    def tree_key(micro, s, t):
        """The word a pair takes in the tree fill's total order (``pc_tree_key``): ``micro << 44 | t << 22 | s``; ``2**64 - 1`` for
        arguments that make no key."""
        return int(load().pc_tree_key(int(micro), int(s), int(t)))

    @staticmethod
    def tree_key_parts(key):
        """``(micro, s, t)`` of a key, or None for a word that is none (``pc_tree_key_parts``)."""
        micro, s, t = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        rc = load().pc_tree_key_parts(int(key), ctypes.byref(micro), ctypes.byref(s), ctypes.byref(t))
        return None if rc != 0 else (int(micro.value), int(s.value), int(t.value))

    def _before_slab_fill(self, metric):
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        self._invalidate_loans()
        return PcStats()

    def _slab_stats(self, kind, stats, **own):
        """The stats dict of such a fill: the fills' summed stats, the call's counts and the kind's two times (affinity: three)."""
        call, *names = self._SLAB_TIMES[kind]
        times = [ctypes.c_float(0.0) for _ in names]
        self._check(getattr(self._lib, call)(self._h, *(ctypes.byref(t) for t in times)))
        return dict(stats.as_dict(), **own, **{name: float(t.value) for name, t in zip(names, times)})

    NEAREST_MAX_K = 64                    # PC_NEAREST_MAX_K: a genome's list lives one entry per lane of a wave

    # -- the rows forms of fill_edges / fill_components / fill_tree / fill_nearest: a stored result grown by new genomes (one GPU) -----------------------
    ROWS_PASSES = ("edges", "components", "tree")

    @staticmethod
    def rows_pass_span(kind):
        """Values one workgroup of the rows pass of ``kind`` (``"edges"``, ``"components"``, ``"tree"``) covers (``pc_rows_pass_span``;
        host arithmetic, no GPU): what a test of the passes' workgroup seams sizes its slabs by."""
        return int(load().pc_rows_pass_span(Context.ROWS_PASSES.index(kind)))

    @staticmethod
    def rows_slabs(n, n_rows, slab_bytes):
        """The slabs a rows form walks for ``n_rows`` query rows of ``n`` genomes under ``slab_bytes`` (> 0): consecutive ranges of
        at most ``max(1, slab_bytes // 8 // n)`` rows (host arithmetic, no GPU)."""
        if int(slab_bytes) <= 0:
            raise ValueError("rows_slabs: slab_bytes must be positive (0 = automatic is decided on the device, by the free HBM)")
        per = max(1, int(slab_bytes) // 8 // max(int(n), 1))
        return (int(n_rows) + per - 1) // per if int(n) > 1 else 0

    _ROWS_CALL = "pc_fill_rows_"

    @staticmethod
    def _rows_arg(rows):
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        return rows, _ptr(rows if rows.size else np.zeros(1, dtype=np.int32), _i32p), int(rows.shape[0])

    @staticmethod
    def _seed_ptr(arr, typ):
        """A seed array for the library: NULL for none and for an empty one."""
        return _ptr(arr, typ) if arr is not None and arr.size else None

    def fill_rows_edges(self, metric, threshold, rows, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """The pairs that touch a query genome of ``rows`` (distinct indices, strictly ascending: the new genomes of a grown
        collection) and pass ``threshold`` (:meth:`fill_edges`' predicate), each once, as ``(src, tgt, val)`` sorted by ``tgt``, then
        ``src``: ``len(rows) * N`` pairs filled instead of ``N (N - 1) / 2``, the whole fill's values.  Merged with a stored list of
        the other genomes' pairs (``matrix.edges_extend``) it is :meth:`fill_edges`' list of the whole collection.  ``slab_bytes`` cuts
        the rows into slabs of ``max(1, slab_bytes // 8 // N)`` (0 = automatic).  Copies, or loans with ``borrow``; ``want_stats`` as
        :meth:`fill_edges`."""
        rows, prow, n_rows = self._rows_arg(rows)
        return self._fill_edge_arrays("edges", self._ROWS_CALL, metric, (int(bool(as_distance)), float(threshold), prow, n_rows, int(slab_bytes)),
                                      want_stats, borrow)

    def fill_rows_components(self, metric, threshold, rows, seed_labels=None, as_distance=True, strict=True, slab_bytes=0, want_stats=False,
                             borrow=False):
        """:meth:`fill_components`' labels of the whole collection from a stored labelling of the other genomes: ``seed_labels``
        (int32[N]: the smallest member of each genome's stored component, a query genome labelling itself; None: every genome its
        own component) is the initial forest, and the passing pairs that touch a query genome of ``rows`` are united into it.
        ``n_edges`` of the stats counts those pairs only."""
        rows, prow, n_rows = self._rows_arg(rows)
        seed = None
        if seed_labels is not None:
            seed = np.ascontiguousarray(seed_labels, dtype=np.int32).reshape(-1)
            if seed.shape[0] != self.n_genomes:
                raise ValueError(f"fill_rows_components: seed_labels holds {seed.shape[0]} entries for {self.n_genomes} genomes")
        return self._fill_labels(self._ROWS_CALL, metric, (int(bool(as_distance)), float(threshold), int(bool(strict)), prow, n_rows,
                                                           self._seed_ptr(seed, _i32p), int(slab_bytes)), want_stats, borrow)

    def fill_rows_tree(self, metric, rows, seed=None, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """:meth:`fill_tree`'s tree of the whole collection from the stored tree of the other genomes: ``seed = (src, tgt, val)``, its
        edges in the uploaded collection's numbering (at most N - 1; values of the call's kind, millionths in [0, 1]), is the
        resident forest the pairs that touch a query genome of ``rows`` are merged into -- MST(A + B) = MST(MST(A) + B).  The
        library refuses a seed that is no key, and a result that does not span the collection."""
        rows, prow, n_rows = self._rows_arg(rows)
        if seed is None:
            seed = ((), (), ())
        s_src = np.ascontiguousarray(seed[0], dtype=np.int32).reshape(-1)
        s_tgt = np.ascontiguousarray(seed[1], dtype=np.int32).reshape(-1)
        s_val = np.ascontiguousarray(seed[2], dtype=np.float64).reshape(-1)
        if not s_src.shape == s_tgt.shape == s_val.shape:
            raise ValueError("fill_rows_tree: the seed's source, target and value arrays differ in length")
        args = (int(bool(as_distance)), prow, n_rows, self._seed_ptr(s_src, _i32p), self._seed_ptr(s_tgt, _i32p), self._seed_ptr(s_val, _f64p),
                int(s_src.shape[0]), int(slab_bytes))
        return self._fill_edge_arrays("tree", self._ROWS_CALL, metric, args, want_stats, borrow)

    @staticmethod
    def nearest_rows_tile():
        """The tile edge of :meth:`fill_rows_nearest`'s column pass (``pc_nearest_rows_tile``; host arithmetic, no GPU): rows and
        columns of the slab a workgroup stages at a time -- what a test of the pass's seams sizes its inputs by."""
        return int(load().pc_nearest_rows_tile())

    def fill_rows_nearest(self, metric, k, rows, seed=None, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """:meth:`fill_nearest`'s lists of the whole collection from the stored lists of the other genomes: ``seed = (nbr, val)``,
        two ``[N, k_seed]`` arrays in the uploaded collection's numbering -- row g of an old genome its best old neighbours, best
        first (rows of the query genomes are ignored) -- replaces the empty lists, and the pairs that touch a query genome of
        ``rows`` are merged into them by the one total order: ``len(rows) * N`` pairs filled instead of ``N (N - 1) / 2``, and
        the result is :meth:`fill_nearest`'s, element for element.  With ``N_old = N - len(rows)`` and ``kk = min(k, N - 1)`` the
        library refuses ``k_seed < min(kk, N_old - 1)``, no seed while ``N_old > 1``, and a seed entry that is out of range, a
        query genome, the genome itself or out of order; columns beyond ``kk`` are cut.  Returns ``(nbr, val)``; ``want_stats``
        adds :meth:`fill_nearest`'s stats (``n_slabs``: the ranges of rows walked).  One GPU."""
        rows, prow, n_rows = self._rows_arg(rows)
        n = self.n_genomes
        s_nbr = s_val = None
        k_seed = 0
        if seed is not None:
            s_nbr = np.ascontiguousarray(seed[0], dtype=np.int32)
            s_val = np.ascontiguousarray(seed[1], dtype=np.float64)
            if s_nbr.ndim != 2 or s_nbr.shape != s_val.shape or s_nbr.shape[0] != n:
                raise ValueError(f"fill_rows_nearest: the seed must be two ({n}, k_seed) arrays, not {s_nbr.shape} and {s_val.shape}")
            k_seed = int(s_nbr.shape[1])
        args = (int(bool(as_distance)), int(k), prow, n_rows, self._seed_ptr(s_nbr, _i32p), self._seed_ptr(s_val, _f64p), k_seed, int(slab_bytes))
        return self._fill_lists(self._ROWS_CALL, metric, args, want_stats, borrow)

    def fill_rows_affinity(self, metric, group, rows, n_groups=None, as_distance=True, slab_bytes=0, want_table=False, want_gain=False,
                           want_stats=False, borrow=False):
        """New genomes placed against the groups of a stored partition: :meth:`fill_affinity`'s statement for the query genomes of
        ``rows`` alone -- ``len(rows) * N`` pairs filled instead of ``N (N - 1) / 2``.  ``group[g]`` in ``[0, n_groups)`` is genome
        g's group or -1: a member of no group (here only; ``n_groups`` defaults to the largest label + 1, at least 1).  Returns a dict
        of arrays over the QUERIES, in the order of ``rows``: ``own_sum`` (int64), ``own_lo``, ``own_hi`` (int32) ``[n_rows]`` -- empty
        for an unlabelled query; ``near_group`` (int32 ``[3, n_rows]``), ``near_sum``, ``near_lo``, ``near_hi`` as :meth:`fill_affinity`
        gives them per genome (an unlabelled query has no own group: every non-empty group is a candidate); ``table``: None, or with
        ``want_table`` the ``(sum, lo, hi)`` of ``[n_rows, G]`` arrays, entry ``[k, b]`` counting ``size[b] - (group[rows[k]] == b)``
        pairs, ``size`` over the labelled genomes, queries included; ``gain``: None, or with ``want_gain`` the ``(sum, lo, hi)`` of
        ``[N]`` arrays -- for an old labelled genome what the queries of its own group add to its own entry (``stored own + gain`` is
        the own entry of :meth:`fill_affinity` over the whole collection), empty elsewhere.  With every genome labelled, query k's
        entries equal entry ``rows[k]`` of :meth:`fill_affinity`'s, integer for integer.  ``as_distance``, ``slab_bytes`` (ranges of
        ``max(1, slab_bytes // 8 // N)`` rows), ``borrow`` and ``want_stats`` (``stats``: with ``n_groups``, ``n_slabs``, ``ms_rows``,
        ``ms_cols``, ``ms_finish``) as there.  One GPU."""
        if group is None:
            raise ValueError("fill_rows_affinity: group is None")
        group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        n = self.n_genomes
        if group.shape[0] != n:
            raise ValueError(f"fill_rows_affinity: group holds {group.shape[0]} labels for {n} genomes")
        if n_groups is None:
            n_groups = max(int(group.max()) + 1, 1) if group.size else 1
        n_groups = int(n_groups)
        rows, prow, n_rows = self._rows_arg(rows)
        pgroup = _ptr(group if group.size else np.zeros(1, dtype=np.int32), _i32p)
        cells = [t() for t in (_i64p, _i32p, _i32p, _i32p, _i64p, _i32p, _i32p, _i64p, _i32p, _i32p, _i64p, _i32p, _i32p)]
        nsl = ctypes.c_int32(0)
        stats = self._slab_call(self._ROWS_CALL + "affinity", metric, int(bool(as_distance)), pgroup, n_groups, prow, n_rows, int(bool(want_table)),
                                int(bool(want_gain)), int(slab_bytes), *(ctypes.byref(c) for c in cells), ctypes.byref(nsl))
        names = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")
        dtypes = (np.int64, np.int32, np.int32, np.int32, np.int64, np.int32, np.int32)
        triple = (np.int64, np.int32, np.int32)
        out = {}
        for name, cell, dtype in zip(names, cells, dtypes):
            shape = (3, n_rows) if name == "near_group" else (n_rows,)
            out[name] = self._lend(cell, shape, borrow) if n_rows and cell else np.empty(shape, dtype=dtype)
        out["table"] = out["gain"] = None
        if want_table:
            out["table"] = tuple(self._lend(cell, (n_rows, n_groups), borrow) if n_rows and cell else np.empty((n_rows, n_groups), dtype=dtype)
                                 for cell, dtype in zip(cells[7:10], triple))
        if want_gain:
            out["gain"] = tuple(self._lend(cell, (n,), borrow) if n and cell else np.empty((n,), dtype=dtype) for cell, dtype in zip(cells[10:], triple))
        if want_stats:
            out["stats"] = self._slab_stats("affinity", stats, n_groups=n_groups, n_slabs=int(nsl.value))
        return out

    def fill_rows_between(self, metric, group, rows, n_groups=None, seed=None, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """A stored between-groups table grown by new genomes: :meth:`fill_between`'s ``(sum, count, lo, hi)`` of the whole collection
        from ``seed`` -- the 4-tuple :meth:`fill_between` gave for the same labels over the genomes that are NOT in ``rows``, in this
        call's direction -- and the pairs that have a query genome of ``rows`` at one end: ``len(rows) * N`` pairs filled instead of
        ``N (N - 1) / 2``, and the result is the whole fill's, integer for integer.  ``group[g]`` in ``[0, n_groups)`` or -1: a member
        of no group, in no pair (``n_groups`` defaults to the largest label + 1, at least 1).  ``seed=None``: the table over the pairs
        with a query end alone.  The library refuses a seed that is not symmetric, not consistent, or whose counts are not the
        partition's own (``old[a] * old[b]``; ``old[a] * (old[a] - 1) / 2`` on the diagonal; ``old`` the labelled genomes outside
        ``rows``), naming the entry.  ``as_distance``, ``slab_bytes`` (ranges of ``max(1, slab_bytes // 8 // N)`` rows), ``borrow``
        and ``want_stats`` as :meth:`fill_between`.  One GPU."""
        if group is None:
            raise ValueError("fill_rows_between: group is None")
        if rows is None:
            raise ValueError("fill_rows_between: rows is None")
        group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        if group.shape[0] != self.n_genomes:
            raise ValueError(f"fill_rows_between: group holds {group.shape[0]} labels for {self.n_genomes} genomes")
        if n_groups is None:
            n_groups = max(int(group.max()) + 1, 1) if group.size else 1
        n_groups = int(n_groups)
        if n_groups < 1:
            raise ValueError(f"fill_rows_between: n_groups {n_groups}")
        pseed = (None, None, None, None)
        if seed is not None:
            if len(seed) != 4 or any(part is None for part in seed):
                raise ValueError("fill_rows_between: seed is the 4-tuple (sum, count, lo, hi) or None")
            seed = [np.ascontiguousarray(part, dtype=dtype) for part, dtype in zip(seed, (np.int64, np.int64, np.int32, np.int32))]
            for name, part in zip(("sum", "count", "lo", "hi"), seed):
                if part.shape != (n_groups, n_groups):
                    raise ValueError(f"fill_rows_between: seed {name} must be {n_groups} x {n_groups} for {n_groups} groups, not {part.shape}")
            pseed = tuple(_ptr(part, typ) for part, typ in zip(seed, (_i64p, _i64p, _i32p, _i32p)))
        rows, prow, n_rows = self._rows_arg(rows)
        pgroup = _ptr(group if group.size else np.zeros(1, dtype=np.int32), _i32p)
        return self._fill_table(self._ROWS_CALL, metric, (int(bool(as_distance)), pgroup, n_groups, prow, n_rows, *pseed, int(slab_bytes)), n_groups,
                                want_stats, borrow)

    def fill_rows_hist(self, metric, rows, group=None, n_groups=None, seed=None, as_distance=True, slab_bytes=0, want_stats=False, borrow=False):
        """A stored histogram grown by new genomes: :meth:`fill_hist`'s array of the whole collection from ``seed`` -- the array
        :meth:`fill_hist` gave for the same labels over the genomes that are NOT in ``rows``, in this call's direction -- and the pairs
        that have a query genome of ``rows`` at one end, each once: ``len(rows) * N`` pairs filled instead of ``N (N - 1) / 2``, and
        the result is the whole fill's, bin for bin.  ``seed=None``: the histogram over the pairs with a query end alone.  The library
        refuses a seed with a negative bin, one whose total is not the old genomes' pair count and, with a partition, one whose row 0
        is not their within count (necessary, not sufficient: a histogram cannot name its pairs).  ``group`` as :meth:`fill_hist`
        (every genome labelled).  ``as_distance``, ``slab_bytes`` (ranges of ``max(1, slab_bytes // 8 // N)`` rows), ``borrow`` and
        ``want_stats`` as :meth:`fill_hist`.  One GPU."""
        if rows is None:
            raise ValueError("fill_rows_hist: rows is None")
        group, pgroup, n_groups = self._hist_group("fill_rows_hist", group, n_groups)
        pseed = None
        if seed is not None:
            classes = 1 if group is None else 2
            seed = np.ascontiguousarray(seed, dtype=np.int64)
            if seed.shape != (classes, HIST_BINS):
                raise ValueError(f"fill_rows_hist: seed must be {classes} x {HIST_BINS}, not {seed.shape}")
            pseed = _ptr(seed, _i64p)
        rows, prow, n_rows = self._rows_arg(rows)
        return self._fill_hist(self._ROWS_CALL, metric, (int(bool(as_distance)), pgroup, n_groups, prow, n_rows, pseed, int(slab_bytes)), want_stats, borrow)

    def fill_rows_dev(self, metric, as_distance, rows, out_ptr, stream=None, want_stats=True):
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        self._check(self._lib.pc_fill_rows_dev(self._h, METRIC_IDS[metric], int(bool(as_distance)), _ptr(rows, _i32p), int(rows.shape[0]),
                                               ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0), ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    def fill_dev(self, metric, as_distance, out_ptr, stream=None, want_stats=True):
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        self._check(self._lib.pc_fill_dev(self._h, METRIC_IDS[metric], int(bool(as_distance)), ctypes.c_void_p(out_ptr),
                                          ctypes.c_void_p(stream or 0), ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    def fill_shard_dev(self, metric, as_distance, shard_ptr, stream=None, want_stats=True):
        stats = PcStats()
        if metric in NEEDS_RESIDUES:
            self.ensure_residues()
        self._check(self._lib.pc_fill_shard_dev(self._h, METRIC_IDS[metric], int(bool(as_distance)),
                                                ctypes.c_void_p(shard_ptr), ctypes.c_void_p(stream or 0),
                                                ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    def assemble_dev(self, gathered_ptr, world, out_ptr, stream=None):
        self._check(self._lib.pc_assemble_dev(self._h, ctypes.c_void_p(gathered_ptr), int(world),
                                              ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)))

    # -- alignment-sliced multi-GPU route (aai / peq): plan everywhere, align a slice, sum to the root, reduce there
    def plan_dev(self, metric, stream=None):
        """Plan the whole (unsharded) aai / peq fill; stats["n_distinct_alignments"] is the length of the result array."""
        stats = PcStats()
        self.ensure_residues()
        self._check(self._lib.pc_plan_dev(self._h, METRIC_IDS[metric], ctypes.c_void_p(stream or 0), ctypes.byref(stats)))
        return stats.as_dict()

    def align_slice_dev(self, slice_rank, slice_world, res_ptr, stream=None, want_stats=True):
        """Align every slice_world-th task of each launch class from slice_rank; 8 bytes per distinct alignment at res_ptr."""
        stats = PcStats()
        self._check(self._lib.pc_align_slice_dev(self._h, int(slice_rank), int(slice_world), ctypes.c_void_p(res_ptr),
                                                 ctypes.c_void_p(stream or 0), ctypes.byref(stats) if want_stats else None))
        return stats.as_dict() if want_stats else None

    def reduce_dev(self, metric, as_distance, res_ptr, out_ptr, stream=None):
        self._check(self._lib.pc_reduce_dev(self._h, METRIC_IDS[metric], int(bool(as_distance)), ctypes.c_void_p(res_ptr),
                                            ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)))

    # -- test hooks --------------------------------------------------------------
    def align_pairs(self, a_gene, b_gene, variant=0, like_fill=False):
        """``variant``: 0 the chooser's, -1 the general kernel, w > 0 the systolic variant of w columns per lane -- with
        ``like_fill`` its buckets cut as a fill cuts them (remainder chooser, small-task modes)."""
        if like_fill and variant > 0:
            variant += 1000
        self.ensure_residues()
        a = np.ascontiguousarray(a_gene, dtype=np.int32)
        b = np.ascontiguousarray(b_gene, dtype=np.int32)
        n = a.shape[0]
        ident, diag = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self._lib.pc_align_pairs(self._h, _ptr(a, _i32p), _ptr(b, _i32p), n, int(variant),
                                             _ptr(ident, _i32p), _ptr(diag, _i32p)))
        return ident, diag

    def set_tie_rule(self, rule):
        """Row of the aligner's tie-rule table (include/phamclust_hip.h); 0 = SURVEY 8c as recalled."""
        self._check(self._lib.pc_set_tie_rule(self._h, int(rule)))

    def tie_rule(self):
        return int(self._lib.pc_get_tie_rule(self._h))

    @staticmethod
    def variant_width(lb):
        """Columns per lane of the systolic variant chosen for a column gene of ``lb`` residues (0: general kernel)."""
        return int(load().pc_variant_width(int(lb)))

    @staticmethod
    def task_shape(lb, width=0):
        """How a column gene of ``lb`` residues runs on the variant of ``width`` columns per lane (0: the chooser's):
        dict of rows per task, waves per workgroup, row streams per wave and strip-mined passes (0: in registers)."""
        out = np.zeros(4, dtype=np.int32)
        if load().pc_task_shape(int(lb), int(width), _ptr(out, _i32p)) != 0:
            raise HipLibraryError(load().pc_last_error().decode())
        return dict(zip(("rows", "waves", "streams", "passes"), out.tolist()))

    @staticmethod
    def ppos_width(max_lb):
        """Columns per lane of the variant a percent-positives launch runs on when its longest column gene has ``max_lb``
        residues (0: general kernel)."""
        return int(load().pc_ppos_width(int(max_lb)))

    WAVE_MODES = 3                      # launch class = base class * WAVE_MODES + mode (0 class's own workgroup, 1 two waves, 2 one wave)

    @staticmethod
    def bucket_launch_classes(lb, rows, any_byte=False):
        """The HOST cut of a bucket of ``rows`` distinct rows against a column gene of ``lb`` residues (``any_byte``: it
        holds a byte outside the alphabet): dict of rows per task, rows kept by the main variant, and the launch classes
        of a full main task, of the last short main task (-1: none) and of the remainder task (-1: none)."""
        out = np.zeros(5, dtype=np.int32)
        if load().pc_bucket_launch_classes(int(lb), int(rows), int(bool(any_byte)), _ptr(out, _i32p)) != 0:
            raise HipLibraryError(load().pc_last_error().decode())
        return dict(zip(("per", "n_main", "full", "last", "rem"), out.tolist()))

    @staticmethod
    def bucket_tasks(lb, rows, any_byte=False):
        """{launch class: tasks} of that bucket, from :meth:`bucket_launch_classes`."""
        cut = Context.bucket_launch_classes(lb, rows, any_byte)
        tasks = {}
        for cls, n in ((cut["full"], cut["n_main"] // cut["per"]), (cut["last"], 1), (cut["rem"], 1)):
            if cls >= 0 and n > 0:
                tasks[cls] = tasks.get(cls, 0) + n
        return tasks

    def last_plan_tasks(self):
        """Tasks per launch class (int32 array) of this context's last aai / peq / aai_ppos fill as the device planner
        cut them, summed over its chunks; after plan_dev the whole plan's, after align_slice_dev that slice's."""
        n = self._lib.pc_last_plan_tasks(self._h, None, 0)
        if n < 0:
            self._check(n)
        out = np.zeros(n, dtype=np.int32)
        self._check(min(0, self._lib.pc_last_plan_tasks(self._h, _ptr(out, _i32p), n)))
        return out

    def last_align_ms(self):
        return float(self._lib.pc_last_align_ms(self._h))

    SET_KERNELS = {0: "popc", 1: "sparse", 2: "sparse64", 3: "walker", 4: "sparsecol", -1: None}

    def last_set_kernel(self):
        """Kernel family the selector gave the last gcs / jc / pocp / af fill (the names PC_SET_KERNEL takes)."""
        return self.SET_KERNELS[int(self._lib.pc_last_set_kernel(self._h))]

    SET_FAMILIES = {name: k for k, name in SET_KERNELS.items() if name}
    SET_METRICS = ("gcs", "jc", "pocp", "af")

    @staticmethod
    def set_kernel_choice(metric, forced=None, **inputs):
        """The selector as host arithmetic (no GPU, no context): the family a fill of ``metric`` runs on for the given
        ``pc_set_inputs`` fields (n, nown, words, two_holder, avg_shared, max_nph, max_ngen, min_gene_len, max_ent_len,
        max_tlen, max_block_entries); ``forced``: a PC_SET_KERNEL name or None."""
        a = PcSetInputs(metric=Context.SET_METRICS.index(metric), forced=-1 if forced is None else Context.SET_FAMILIES[forced], **inputs)
        k = load().pc_set_kernel_choice(ctypes.byref(a))
        if k < 0:
            raise HipLibraryError(load().pc_last_error().decode())
        return Context.SET_KERNELS[k]

    @staticmethod
    def set_launch_shape(family, metric, n, nown, words, two_holder, n_cu=256, table_top=0, popc_tile=0, s64_chunks=0, col_seg=0):
        """Launch shape (dict, see ``pc_set_shape``) of ``family`` for that fill; the last three are the values of the
        PC_POPC_TILE / PC_S64_CHUNKS / PC_COL_SEG knobs (0: unset).  Host arithmetic, no GPU."""
        out, knobs = PcSetShape(), np.array([popc_tile, s64_chunks, col_seg], dtype=np.int32)
        if load().pc_set_launch_shape(Context.SET_FAMILIES[family], Context.SET_METRICS.index(metric), int(n), int(nown), int(words),
                                      int(two_holder), int(n_cu), int(table_top), _ptr(knobs, _i32p), ctypes.byref(out)) != 0:
            raise HipLibraryError(load().pc_last_error().decode())
        d = out.as_dict()
        d["family"] = family
        return d

    @staticmethod
    def set_max_block_entries(entries_per_genome, owned):
        """``max_block_entries`` of the selector's inputs as the fills count it (host arithmetic, no GPU): the most entries in
        a block of 64 consecutive owned targets, the ragged last block included."""
        per = np.ascontiguousarray(entries_per_genome, dtype=np.uint32)
        owned = np.ascontiguousarray(owned, dtype=np.int32)
        n = load().pc_set_max_block_entries(_ptr(per, ctypes.POINTER(ctypes.c_uint32)), _ptr(owned, _i32p), owned.shape[0])
        if n < 0:
            raise HipLibraryError(load().pc_last_error().decode())
        return int(n)

    def last_set_launch(self):
        """(selector inputs, launch shape) of this context's last gcs / jc / pocp / af fill, as two dicts; names instead of
        ids for metric, forced and family."""
        a, shape = PcSetInputs(), PcSetShape()
        self._check(self._lib.pc_last_set_launch(self._h, ctypes.byref(a), ctypes.byref(shape)))
        a, shape = a.as_dict(), shape.as_dict()
        a["metric"], a["forced"] = self.SET_METRICS[a["metric"]], self.SET_KERNELS[a["forced"]]
        shape["family"] = self.SET_KERNELS[shape["family"]]
        return a, shape

    @staticmethod
    def chunk_plan(counts, max_per_chunk):
        """The chunking rule of memory-bounded fills (host arithmetic in the library; no GPU): range starts + [n]."""
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        cuts = np.zeros(counts.shape[0] + 2, dtype=np.int32)
        n = load().pc_chunk_plan(_ptr(counts, _u64p), counts.shape[0], int(max_per_chunk), _ptr(cuts, _i32p), cuts.shape[0])
        if n < 0:
            raise HipLibraryError(load().pc_last_error().decode())
        return cuts[:n + 1]

    def round6(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        out = np.empty_like(v)
        self._check(self._lib.pc_round6_probe(self._h, _ptr(v, _f64p), _ptr(out, _f64p), v.shape[0]))
        return out


class MultiContext(_SlabFills):
    """Several GPUs of this node driven from THIS process (``pc_multi_*``: a context and a host thread per device inside the
    library, the shard exchange as device-to-device copies) -- the multi-GPU route that costs no launcher, no interpreter and no
    process group per GPU.  ``device_ids[0]`` delivers the matrix; an id may repeat (several contexts on one GPU: rehearsal).
    Same surface as :class:`Context` where it matters to ``matrix_de_novo``: ``upload`` / ``fill``."""

    def __init__(self, device_ids):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self._packed = None
        self.device_ids = [int(x) for x in device_ids]
        ids = np.ascontiguousarray(self.device_ids, dtype=np.int32)
        rc = self._lib.pc_multi_create(ctypes.byref(self._h), _ptr(ids, _i32p), int(ids.shape[0]))
        if rc != 0:
            # (the other multi-GPU route starts fresh CHILD processes, one per GPU; this process is never re-executed)
            raise HipLibraryError(f"libphamclust_hip: status {rc}: {self._lib.pc_last_error().decode()} -- devices {self.device_ids} could not "
                                  f"all be opened from one process; PHAMCLUST_MULTI=launcher runs the same shard as one process per GPU "
                                  f"(torch.distributed.run, one RCCL gather)")

    PEER_ACCESS = {2: "same-device", 1: "peer", 0: "staged (no peer access)", -1: "staged (peer access failed)"}

    def peer_access(self):
        """How each device's shard reaches ``device_ids[0]``: a list of ``{"device", "access", "code"}`` plus the runtime's reasons
        for every copy that is NOT device to device (``pc_multi_peer_access``).  Never silent: ``fill`` stats and the CLI log carry it."""
        codes = np.zeros(self.n_devices, dtype=np.int32)
        staged = self._lib.pc_multi_peer_access(self._h, _ptr(codes, _i32p))
        if staged < 0:
            self._check(staged)
        note = self._lib.pc_last_error().decode().strip() if staged else ""
        return {"devices": [{"device": d, "code": int(c), "access": self.PEER_ACCESS[int(c)]} for d, c in zip(self.device_ids, codes)],
                "staged_through_host": int(staged), "note": note}

    _check = Context._check
    _struct = staticmethod(Context._struct)
    _invalidate_loans = Context._invalidate_loans
    _lend = Context._lend

    @property
    def n_devices(self):
        return len(self.device_ids)

    @property
    def n_pairs(self):
        return self._packed.n_pairs

    @property
    def n_genomes(self):
        return self._packed.n_genomes

    def close(self):
        self._invalidate_loans()
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.pc_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:                                          # noqa: BLE001 -- interpreter shutdown
            pass

    def upload(self, packed, residues=True):
        packed.validate()
        s = self._struct(packed)
        self._invalidate_loans()
        self._check(self._lib.pc_multi_upload(self._h, ctypes.byref(s), int(bool(residues))))
        self._packed, self._residues = packed, bool(residues)
        return self

    def set_tie_rule(self, rule):
        self._check(self._lib.pc_multi_set_tie_rule(self._h, int(rule)))

    def fill(self, metric, as_distance=True, want_stats=False, borrow=True):
        """The whole matrix over all devices: condensed f64 vector (a loan of the root context's pinned memory, like
        ``Context.fill(borrow=True)``; ``borrow=False`` copies it).  Stats: the root device's fill plus ``per_device`` (every
        device's own), ``ms_exchange`` (slowest device-to-root copy), ``ms_assemble``."""
        if self._packed is None:
            raise HipLibraryError("no genomes uploaded")
        if metric in NEEDS_RESIDUES and not self._residues:
            s = self._struct(self._packed)
            self._check(self._lib.pc_multi_upload_residues(self._h, ctypes.byref(s)))
            self._residues = True
        self._invalidate_loans()
        stats = (PcStats * self.n_devices)()
        ptr, x_ms, a_ms = _f64p(), ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._lib.pc_multi_fill_borrow(self._h, METRIC_IDS[metric], int(bool(as_distance)), ctypes.byref(ptr), stats,
                                                   ctypes.byref(x_ms), ctypes.byref(a_ms)))
        out = self._lend(ptr, (max(self.n_pairs, 1),))[:self.n_pairs]
        if not borrow:
            out = out.copy()
        if not want_stats:
            return out
        per = [s.as_dict() for s in stats]
        merged = dict(per[0], per_device=per, ms_exchange=float(x_ms.value), ms_assemble=float(a_ms.value), n_devices=self.n_devices,
                      ms_total=max(p["ms_total"] for p in per), peer_access=self.peer_access())
        return out, merged

    # -- the fills that deliver no dense matrix, over all devices (_SlabFills: pc_multi_fill_edges / _components / _nearest / _tree) ----
    _SLAB_CALL = "pc_multi_fill_"

    def _tree_rounds(self):
        """(the round counts are a single context's: ``pc_last_tree_rounds`` takes one)"""
        return {}

    @staticmethod
    def slab_stretches(cost, world):
        """The deal of those fills as host arithmetic (``pc_stretch_plan``; no GPU): ``bounds[world + 1]`` -- device r walks the
        contiguous targets ``[bounds[r], bounds[r + 1])``, stretches of about equal summed ``cost`` (uint64 per target: ``t`` for
        gcs / jc / pocp / af, ``target_costs()[t] + 2000 * t`` for aai / peq); a stretch may be empty."""
        cost = np.ascontiguousarray(cost, dtype=np.uint64).reshape(-1)
        bounds = np.zeros(int(world) + 1 if int(world) >= 1 else 1, dtype=np.int32)
        lib = load()
        if lib.pc_stretch_plan(_ptr(cost if cost.size else np.zeros(1, np.uint64), _u64p), int(cost.shape[0]), int(world), _ptr(bounds, _i32p)) != 0:
            raise HipLibraryError(lib.pc_last_error().decode())
        return bounds

    def _before_slab_fill(self, metric):
        """What the four calls share ahead of the library call: the residues on demand, earlier loans ended, a stats array."""
        if self._packed is not None and metric in NEEDS_RESIDUES and not self._residues:     # (before an upload the library refuses the call itself)
            s = self._struct(self._packed)
            self._check(self._lib.pc_multi_upload_residues(self._h, ctypes.byref(s)))
            self._residues = True
        self._invalidate_loans()
        return (PcStats * self.n_devices)()

    def _slab_stats(self, kind, stats, **own):
        """The stats dict of such a fill: the counts summed over the devices, the times of the slowest, and what the route adds --
        ``n_devices``, ``per_device``, ``stretches``, ``ms_exchange``, ``ms_merge``, ``peer_access``."""
        per = [s.as_dict() for s in stats]
        merged = {name: (max if name.startswith("ms_") else sum)(p[name] for p in per) for name in per[0]}
        bounds = np.zeros(self.n_devices + 1, dtype=np.int32)
        self._check(self._lib.pc_multi_last_stretches(self._h, _ptr(bounds, _i32p)))
        x, y = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._lib.pc_multi_last_slab_times(self._h, ctypes.byref(x), ctypes.byref(y)))
        return dict(merged, **own, n_devices=self.n_devices, per_device=per, stretches=bounds.tolist(), ms_exchange=float(x.value),
                    ms_merge=float(y.value), peer_access=self.peer_access())
