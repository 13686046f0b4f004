"""CPU tests of the host side: Genome / SymMatrix surface, packing, synthetic data,
TSV I/O, the C-ABI export list, and loud failure without the HIP library."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, golden_file, read_lower_triangle


# ---- Genome ---------------------------------------------------------------------------
def test_genome_surface():
    from phamclust_amd.genome import Genome
    g = Genome("g1")
    g.add("p1", "MKV"); g.add("p2"); g.add("p1", "MKL")
    assert g.phams == {"p1": ["MKV", "MKL"], "p2": ["M"]}
    assert len(g) == 3 and len(g.phams) == 2 and "p1" in g and "zz" not in g
    assert g["p1"] == ["MKV", "MKL"]
    with pytest.raises(KeyError):
        g["zz"]
    with pytest.raises(TypeError):
        g.add(1, "M")
    with pytest.raises(TypeError):
        g.add("p", 5)
    with pytest.raises(TypeError):
        1 in g
    h = Genome("g2"); h.add("p2", "MA"); h.add("p3", "MC")
    assert g & h == {"p2"} == g.intersection(h)
    assert g | h == {"p1", "p2", "p3"} == g.union(h)
    assert g - h == {"p1"} == g.difference(h)
    assert g ^ h == {"p1", "p3"} == g.symmetric_difference(h)
    with pytest.raises(TypeError):
        g & "x"
    assert str(g) == ">name=g1|pham=p1|n=1\nMKV\n>name=g1|pham=p1|n=2\nMKL\n>name=g1|pham=p2|n=1\nM\n"
    assert h < g and g.pop("p2") == ["M"] and g.pop("p2") is None


def test_genome_fasta_roundtrip(tmp_path):
    from phamclust_amd.genome import Genome, GenomeLoadError
    g = Genome("g1"); g.add("p1", "MKV"); g.add("p1", "MKL"); g.add("p9", "MW")
    path = g.save(tmp_path / "g1.fasta")
    h = Genome("g1"); h.load(path)
    assert h.phams == g.phams
    bad = tmp_path / "bad.fasta"
    bad.write_text(">name=x|n=1\nMK\n")
    with pytest.raises(GenomeLoadError):
        Genome("x").load(bad)


# ---- packing --------------------------------------------------------------------------
def test_pack_layout(small_genomes, small_packed):
    pk = small_packed
    assert pk.names == [g.name for g in small_genomes] == sorted(pk.names)
    assert pk.n_phams == len({p for g in small_genomes for p in g.phams})
    for i, g in enumerate(small_genomes):
        assert pk.nph[i] == len(g.phams) and pk.ngen[i] == len(g)
        assert pk.tlen[i] == sum(len(t) for ts in g.phams.values() for t in ts)
        ids = pk.gene_pham[pk.gene_off[i]:pk.gene_off[i + 1]]
        assert (np.diff(ids) >= 0).all()
        row = pk.bitmap[i * pk.words_per_row:(i + 1) * pk.words_per_row]
        assert sum(bin(int(w)).count("1") for w in row) == len(g.phams)
    from phamclust_amd.pack import unpack_genomes
    back = unpack_genomes(pk)
    for g, h in zip(small_genomes, back):
        assert {p: ts for p, ts in g.phams.items()} == {p: ts for p, ts in h.phams.items()}


def test_pack_rejects_empty_and_wide_chars():
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    with pytest.raises(ValueError):
        pack_genomes([])
    g = Genome("g"); g.add("p", "MK中")
    with pytest.raises(ValueError):
        pack_genomes([g])


def test_synth_is_deterministic_and_consistent(native_built):
    from phamclust_amd.pack import pack_genomes, unpack_genomes
    from phamclust_amd.synth import synth_packed
    a, b = synth_packed(50, 700), synth_packed(50, 700)
    for f in ("bitmap", "nph", "ngen", "tlen", "gene_off", "gene_pham", "seq_off", "residues"):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    c = synth_packed(50, 700, seed=1)
    assert not np.array_equal(a.residues[:1000], c.residues[:1000])
    again = pack_genomes(unpack_genomes(a))          # the generator's packing == pack_genomes of its genomes
    for f in ("bitmap", "nph", "ngen", "tlen", "gene_off", "gene_pham", "seq_off", "residues"):
        assert np.array_equal(getattr(a, f), getattr(again, f))
    assert a.names[0] == "synth_000000" and 60 <= a.nph.min() and a.nph.max() <= 140
    lens = np.diff(a.seq_off)
    assert lens.min() >= 1 and lens.max() <= 1500 and 150 < lens.mean() < 280
    assert set(np.unique(a.residues).tolist()) <= set(map(ord, "ACDEFGHIKLMNPQRSTVWY"))


# ---- SymMatrix ------------------------------------------------------------------------
def _toy():
    from phamclust_amd.matrix import SymMatrix
    m = SymMatrix(["b", "a", "c"], is_distance=True)
    for n in "abc":
        m.set_weight(n, n, 0.0)
    m.set_weight("a", "b", 0.1234564)
    m.set_weight("c", "a", 0.5)
    m.set_weight("b", "c", 0.9)
    return m


def test_symmatrix_basic_surface():
    m = _toy()
    assert len(m) == 3 and m.nodes == ["b", "a", "c"] and m.is_distance
    assert m.get_weight("b", "a") == m.get_weight("a", "b") == 0.123456          # rounded on write
    assert list(m) == [("b", "b", 0.0), ("b", "a", 0.123456), ("b", "c", 0.9),
                       ("a", "a", 0.0), ("a", "c", 0.5), ("c", "c", 0.0)]
    assert [r for _, r in m.iterrows()] == [[0.0, 0.123456, 0.9], [0.123456, 0.0, 0.5], [0.9, 0.5, 0.0]]
    assert m["a"] == {"a": 0.0, "b": 0.123456, "c": 0.5} and m["c"] == {"c": 0.0}  # string-ordered keys
    with pytest.raises(ValueError):
        m.set_weight("a", "b", 1.5)
    with pytest.raises(KeyError):
        m.set_weight("a", "zz", 0.5)
    with pytest.raises(KeyError):
        m.get_weight("zz", "a")
    with pytest.raises(TypeError):
        5 in m
    m.lock()
    with pytest.raises(AttributeError):
        m.set_weight("a", "b", 0.2)
    assert m.is_locked()
    m.unlock()
    assert m.diameter == 0.9
    assert np.array_equal(m.to_ndarray(condensed=True), np.array([0.123456, 0.9, 0.5]))
    assert str(m).splitlines()[0] == "3" and str(m).splitlines()[1].startswith("b" + " " * 23 + "\t0.000000\t0.123456")
    from phamclust_amd.matrix import SymMatrix
    assert SymMatrix(["x"]) < m
    unset = SymMatrix(["x", "y"])
    assert unset.get_weight("x", "y") is None


def test_symmatrix_medoid_invert_extract_reorder():
    from phamclust_amd.matrix import SymMatrix
    m = _toy()
    # medoid: mean over N+1 incident weights with the diagonal counted twice, ties by node order
    central = {"b": (0.0 + 0.0 + 0.123456 + 0.9) / 4, "a": (0.123456 + 0.0 + 0.0 + 0.5) / 4, "c": (0.9 + 0.5 + 0.0 + 0.0) / 4}
    assert m.medoid[0] == "a" and m.medoid[1] == pytest.approx(central["a"])
    assert m.anti_medoid[0] == "c"
    sub = m.extract_submatrix(["c", "a"])
    assert sub.nodes == ["c", "a"] and sub.get_weight("a", "c") == 0.5 and sub.is_distance
    with pytest.raises(KeyError):
        m.extract_submatrix(["a", "zz"])
    m.invert()
    assert not m.is_distance and m.get_weight("a", "b") == 0.876544 and m.get_weight("a", "a") == 1.0
    assert m.medoid[0] == "a"                       # similarity: largest mean
    with pytest.raises(ValueError):
        m.diameter
    m.invert()
    m.reorder(["a", "b", "c"])
    assert m.nodes == ["a", "b", "c"] and list(m)[1] == ("a", "b", 0.123456)
    with pytest.raises(ValueError):
        m.reorder(["a", "b"])
    m.reorder()                                     # single-linkage tree order
    assert sorted(m.nodes) == ["a", "b", "c"]
    assert m.nearest_neighbors("a", 0.6) == ["b", "c"]
    m.append_node("d", {"a": 0.2, "b": 0.3, "c": 0.4, "d": 0.0})
    assert len(m) == 4 and m.get_weight("d", "b") == 0.3
    with pytest.raises(KeyError):
        m.append_node("d", {"a": 0.2, "b": 0.3, "c": 0.4, "d": 0.0})
    with pytest.raises(ValueError):
        m.append_node("e", {"a": 0.2, "b": 0.3, "c": 0.4, "d": 0.1, "e": 1.0})
    mean, sd, skew = m.statistics
    assert mean == pytest.approx(np.mean([0.123456, 0.5, 0.9, 0.2, 0.3, 0.4]))
    one = SymMatrix(["x"], True); one.set_weight("x", "x", 0.0)
    assert one.statistics == (0.0, 0.0, 0.0)


def test_from_condensed_and_tsv_roundtrip(tmp_path):
    from phamclust_amd.matrix import (SymMatrix, matrix_from_adjacency, matrix_from_squareform,
                                      matrix_to_adjacency, matrix_to_squareform)
    names, gold, diag = read_lower_triangle(golden_file("jc"))
    m = SymMatrix.from_condensed(names, gold, is_distance=True)
    assert np.array_equal(m.to_ndarray(condensed=True), gold)
    # lower-triangle writer is byte-identical to the file the reference wrote
    out = matrix_to_squareform(m, tmp_path / "lt.tsv", lower_triangle=True)
    assert open(out).read() == open(golden_file("jc")).read()
    back = matrix_from_squareform(out)
    assert back.is_distance and back.nodes == names and np.array_equal(back.to_ndarray(condensed=True), gold)
    full = matrix_to_squareform(m, tmp_path / "sq.tsv")
    assert open(full).readline().rstrip().split("\t") == [str(len(names))] + names
    assert np.array_equal(matrix_from_squareform(full).to_ndarray(condensed=True), gold)
    m.invert()
    adj = matrix_to_adjacency(m, tmp_path / "adj.tsv")
    assert open(adj).read() == open(golden_file("jc", "similarity")).read()
    again = matrix_from_adjacency(adj)
    assert not again.is_distance and np.array_equal(again.to_ndarray(), m.to_ndarray())
    with pytest.raises(ValueError):
        SymMatrix.from_condensed(names, gold[:-1])


def test_matrix_de_novo_generic_callable_and_errors():
    from phamclust_amd.genome import Genome
    from phamclust_amd.matrix import _outside_in_index_iterator, matrix_de_novo
    assert list(_outside_in_index_iterator(5)) == [0, 4, 1, 3, 2]          # reference matrix.py:415-416
    assert list(_outside_in_index_iterator(4)) == [0, 3, 1, 2] and list(_outside_in_index_iterator(1)) == [0]
    with pytest.raises(ValueError):
        matrix_de_novo([], lambda s, t, as_distance=False: 0.0, 1)
    gs = []
    for k in range(4):
        g = Genome(f"g{k}")
        for p in range(k + 1):
            g.add(f"p{p}")
        gs.append(g)

    def overlap(source, target, as_distance=False):       # any user callable: generic per-pair path
        sim = len(source & target) / 4.0
        return round(1.0 - sim, 6) if as_distance else round(sim, 6)

    m = matrix_de_novo(gs, overlap, 2)
    assert m.is_distance and m.get_weight("g0", "g3") == 0.75 and m.get_weight("g2", "g3") == 0.25
    assert all(m.get_weight(g.name, g.name) == 0.0 for g in gs)
    sim = matrix_de_novo(gs, overlap, 1, as_distance=False)
    assert not sim.is_distance and sim.get_weight("g1", "g1") == 1.0 and sim.get_weight("g1", "g2") == 0.5


def _toy_shared_fraction(source, target, as_distance=False):
    """A metric that is none of the six METRICS: matrix_de_novo's generic path (module level: joblib pickles it by name)."""
    union = len(source | target)
    sim = len(source & target) / union if union else 0.0
    return round(1.0 - sim, 6) if as_distance else round(sim, 6)


def test_generic_callable_over_cpus_equals_one_process(native_built):
    """matrix.py:471-493: ANY callable is spread over `cpus` workers.  cpus=2 (joblib, unordered results) must give the
    matrix cpus=1 gives, for plain genomes and for the C loader's lazy genomes (which pickle as plain ones and stay lazy)."""
    import random
    from phamclust_amd.genome import Genome
    from phamclust_amd.matrix import matrix_de_novo
    from phamclust_amd.pack import load_tsv_genomes, packed_behind
    rng = random.Random(5)
    gs = []
    for k in range(37):
        g = Genome(f"g{k:02d}")
        for p in rng.sample(range(60), rng.randint(1, 25)):
            g.add(f"p{p}", "MK" * rng.randint(1, 4))
        gs.append(g)
    one = matrix_de_novo(gs, _toy_shared_fraction, 1)
    two = matrix_de_novo(gs, _toy_shared_fraction, 2)
    assert one.nodes == two.nodes and np.array_equal(one.to_ndarray(), two.to_ndarray())
    assert len({one.get_weight(a.name, b.name) for a in gs for b in gs}) > 20        # not a constant matrix
    lazy = load_tsv_genomes(os.path.join(REPO, "tests", "golden", "small_input.tsv"))
    m1 = matrix_de_novo(lazy, _toy_shared_fraction, 1, as_distance=False)
    assert packed_behind(lazy) is None                          # cpus=1 read .phams in this process: detached
    lazy = load_tsv_genomes(os.path.join(REPO, "tests", "golden", "small_input.tsv"))
    m3 = matrix_de_novo(lazy, _toy_shared_fraction, 3, as_distance=False)
    assert packed_behind(lazy) is not None                      # the workers got plain copies; the originals stayed lazy
    assert np.array_equal(m1.to_ndarray(), m3.to_ndarray())
    # more workers than pairs: clamped like the reference (matrix.py:460-462)
    tiny = matrix_de_novo(gs[:2], _toy_shared_fraction, 64)
    assert tiny.get_weight("g00", "g01") == one.get_weight("g00", "g01")


def test_cli_surface():
    from phamclust_amd import cli
    assert list(cli.METRICS) == ["gcs", "jc", "pocp", "af", "aai", "peq"]
    args = cli.parse_args(["in.tsv", "out"])
    assert args.metric == "peq" and args.nr_thresh == 0.75 and args.clu_thresh == 0.25 and args.sub_thresh == 0.6
    assert args.nr_linkage == "complete" and args.clu_linkage == "average" and args.sub_linkage == "single" and args.k_min == 6
    assert cli.parse_args(["in.tsv", "out", "-m", "jc", "-t", "3"]).metric == "jc"
    assert args.device is None and args.gpus == 1 and cli.parse_args(["in.tsv", "out", "--device", "3"]).device == 3
    with pytest.raises(SystemExit):
        cli.parse_args(["in.tsv", "out", "-m", "nope"])


# ---- C-ABI ------------------------------------------------------------------------------
def test_abi_exports_match_header(native_built):
    """The library loads and exports exactly the functions include/phamclust_hip.h declares
    (no compute calls here: there is no GPU on the CPU box)."""
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    declared = set(re.findall(r"\b(pc_[a-z0-9_]+)\s*\(", header)) - {"pc_ctx"}
    assert declared == set(hip.EXPORTS)
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert hip.load().pc_version() == int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 110
    # the release library carries no fault injection; its -DPC_TEST_HOOKS twin exports the same ABI and says what it is
    assert hip.load().pc_test_hooks() == 0
    twin = ctypes.CDLL(os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so"))
    for name in declared:
        assert hasattr(twin, name), name
    assert twin.pc_test_hooks() == 1 and twin.pc_version() == hip.load().pc_version()
    assert b"PC_FAKE_OOM_ABOVE" not in open(hip.LIB_PATH, "rb").read()
    assert ctypes.sizeof(hip.PcPacked) == 16 + 8 * 8 and ctypes.sizeof(hip.PcStats) == 5 * 8 + 2 * 4 + 4 * 4 + 2 * 8
    assert "n_chunks" in hip.PcStats().as_dict()


def test_task_shape_and_percent_positives_route(native_built):
    """The host-side launch arithmetic that tests/test_gpu_limits.py builds its cases on (no GPU call): strip passes of a
    65,535-residue column gene per wide variant, a full task of a 100-residue column on W = 2 / 3 (one row stream per wave,
    52 alignments each), and where percent-positives leaves the strip-mined profile cell (13-bit fields: 8,191 columns)."""
    from phamclust_amd import hip
    C = hip.Context
    assert [C.task_shape(65535, w)["passes"] for w in (32, 48, 64)] == [32, 22, 16]
    assert C.task_shape(4096, 32)["passes"] == 2 and C.task_shape(4097, 32)["passes"] == 3 and C.task_shape(4096, 64)["passes"] == 0
    for w in (2, 3):
        assert C.task_shape(100, w) == {"rows": 208, "waves": 4, "streams": 1, "passes": 0}
    assert C.task_shape(100, 4)["streams"] == 2
    assert [C.ppos_width(n) for n in (1536, 1537, 7681, 8191, 8192, 9000)] == [24, 24, 24, 24, 0, 0]
    for lb, w in ((100, 1), (65536, 0), (0, 0)):
        with pytest.raises(hip.HipLibraryError):
            C.task_shape(lb, w)
    # the bucket hook agrees with the shape hook: same task size, and a bucket of exactly one wave round / one task is one task
    for lb in (1, 100, 650, 1536, 1537, 4096, 4097, 65535):
        shape, cut = C.task_shape(lb), C.bucket_launch_classes(lb, C.task_shape(lb)["rows"])
        assert cut["per"] == cut["n_main"] == shape["rows"] and cut["last"] == cut["rem"] == -1 and cut["full"] % 3 == (2 if shape["rows"] <= shape["streams"] else 0)
        assert C.bucket_tasks(lb, shape["streams"]) == {cut["full"] - cut["full"] % 3 + 2: 1}
    assert hip.load().pc_last_plan_tasks(None, None, 0) == hip.load().pc_bucket_launch_classes(100, 1, 0, None) == -1       # PC_ERR_ARG


def test_bucket_launch_classes_hook(native_built):
    """pc_bucket_launch_classes, the host cut of one bucket (no GPU call): task size, rows kept by the main variant and the
    launch classes of a full, a last and a remainder task, at shapes worked out by hand from pc_nw_shape.hip; pc_last_plan_tasks
    refuses a NULL context."""
    from phamclust_amd import hip
    C = hip.Context
    # 100 residues: W = 13 (variant index 11), 8 lanes per segment (bucket <= 8), 8 segments per wave -> base class 11 * 4 + 0
    cut = C.bucket_launch_classes(100, 208 + 8, False)
    assert cut["per"] == 208 and cut["n_main"] == 216 and cut["full"] == 44 * 3 and cut["last"] == 44 * 3 + 2 and cut["rem"] == -1
    assert C.bucket_tasks(100, 208 + 8) == {44 * 3: 1, 44 * 3 + 2: 1}
    assert C.bucket_launch_classes(100, 16, False)["last"] == 44 * 3 + 1        # 2 x 8 rows: two waves
    assert C.bucket_launch_classes(100, 16, True)["last"] == (24 * 4 + 44) * 3 + 1      # the "any byte" classes lie 24 x 4 higher
    # a moved remainder: 9 = 8 + 1 rows; the single left-over row goes to the cheapest step with one segment, W = 2 on 50 lanes
    # (variant 0, bucket <= 64), in a one-wave workgroup
    cut = C.bucket_launch_classes(100, 9, False)
    assert cut["n_main"] == 8 and cut["last"] == 44 * 3 + 2 and cut["rem"] == (0 * 4 + 3) * 3 + 2
    assert C.bucket_launch_classes(100, 9, True)["rem"] == (24 * 4 + 3) * 3 + 2
    # 650 residues: W = 32 takes any byte itself and keeps its class; its remainder variant (W = 11) does not
    clean, odd = C.bucket_launch_classes(650, 4, False), C.bucket_launch_classes(650, 4, True)
    assert clean["full"] == odd["full"] and clean["rem"] == (9 * 4 + 3) * 3 + 2 and odd["rem"] == clean["rem"] + 24 * 4 * 3
    # strip-mined: one row per wave, four rows per task; classes follow the 2 x 24 x 4 systolic ones
    assert C.bucket_tasks(4097, 9) == {192 * 3: 2, 192 * 3 + 2: 1} and C.bucket_tasks(8193, 2, True) == {193 * 3 + 1: 1}
    for lb, rows in ((0, 1), (65536, 1), (10, 0)):
        with pytest.raises(hip.HipLibraryError):
            C.bucket_launch_classes(lb, rows)
    assert hip.load().pc_last_plan_tasks(None, None, 0) == -1


# launch classes no collection reaches in a default process (each with its reason); tests/test_gpu_planner.py's collection
# must reach every other one
UNREACHED_BY_DESIGN = {
    195 * 3: "general kernel: needs PC_STRIP=0 or percent-positives beyond 8,191 columns (test_launch_policy_switches_change_no_value, tests/test_gpu_limits.py)",
    194 * 3: "strip-mined W = 64: the chooser's cost model never prefers 4,096-column passes for a gene of up to 65,535 residues; forced in tests/test_gpu_limits.py",
    194 * 3 + 1: "strip-mined W = 64, two waves: as above",
    194 * 3 + 2: "strip-mined W = 64, one wave: as above",
}


def test_planner_collection_reaches_every_launch_class(native_built):
    """The collection tests/test_gpu_planner.py drives through the fills covers the device planner's choices: the launch
    classes the host cut predicts for its buckets EQUAL the reachable set -- every class pc_bucket_launch_classes returns for
    a column of 1 ... 4,096 residues with 1 ... 2 x 208 + 16 rows, clean or not, plus the strip-mined classes in the modes
    pc_task_shape gives them and the general kernel -- except the classes listed above.  Fails, naming the class, when a
    variant, a tier or a mode is added without a case that reaches it, or when a case that alone reached one is dropped."""
    import planner_cases as pc
    from phamclust_amd import hip
    C = hip.Context
    lib, out = hip.load(), np.zeros(5, dtype=np.int32)
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    reachable = set()
    for lb in range(1, pc.MAX_LB + 1):
        for any_byte in (0, 1):
            for rows in range(1, pc.MAX_ROWS + 1):
                assert lib.pc_bucket_launch_classes(lb, rows, any_byte, ptr) == 0
                per, n_main, full, last, rem = out.tolist()
                reachable.update(c for c in (full if n_main >= per else -1, last, rem) if c >= 0)
    n_systolic = 24 * 8 * 3
    assert max(reachable) < n_systolic
    for k, w in enumerate((32, 48, 64)):                                     # a gene beyond the variant's 64 x W columns: one row per wave
        rows = C.task_shape(64 * w + 1, w)["rows"]
        assert C.task_shape(64 * w + 1, w)["passes"] == 2 and rows >= 3
        reachable.update(n_systolic + 3 * k + mode for mode in range(3))    # (<= 1 row: one wave, <= 2: two waves, else the class's workgroup)
    reachable.add(n_systolic + 9)                                           # the general kernel has no small-task modes
    cases = pc.design(C)
    reached = pc.classes_of(C, cases)
    assert len(UNREACHED_BY_DESIGN) == 4 and set(UNREACHED_BY_DESIGN) <= reachable
    missing = reachable - set(reached) - set(UNREACHED_BY_DESIGN)
    assert not missing, "no case of the collection reaches: " + "; ".join(f"{c} ({pc.class_name(C, c)})" for c in sorted(missing))
    assert set(reached) == reachable - set(UNREACHED_BY_DESIGN), sorted(set(reached) - reachable)
    # the check has teeth: without the cases of 650 residues' neighbours (the W = 32 island at 641 ... 672) classes go missing
    fewer = pc.classes_of(C, [case for case in cases if not 641 <= case[0] <= 672])
    assert reachable - set(fewer) - set(UNREACHED_BY_DESIGN)
    assert all(1 <= lb <= 65535 and 1 <= rows <= pc.MAX_ROWS for lb, rows, _ in cases)


# ---- the set-metric selector and its launch shapes (host arithmetic of pc_set_shape.hip) -----------------------
def _choice_base(**over):
    """synth(N, 5000)'s profile: 79 bitmap words, 5,000 phams with two holders (5,056 mask entries), 2.85 phams shared per pair;
    blocks of 6,500 entries against the value table's 7,231 at that mask count."""
    base = dict(n=3000, nown=3000, words=79, two_holder=5000, avg_shared=2.85, max_nph=140, max_ngen=160, min_gene_len=1,
                max_ent_len=3000, max_tlen=40000, max_block_entries=6500)
    base.update(over)
    return base


def test_set_kernel_choice_pins(native_built):
    """pc_set_kernel_choice, the selector as a function of its inputs (no GPU, no context), on both sides of every threshold and
    guard of pick_set_kernel -- worked out by hand from pc_set_shape.hip, not read off the function."""
    from phamclust_amd import hip
    C = hip.Context

    def pick(metric, forced=None, **over):
        side = over.pop("side", None)
        if side is not None:
            over.update(n=side, nown=side)
        return C.set_kernel_choice(metric, forced=forced, **_choice_base(**over))
    # the column kernel's area: 2,200^2 (gcs / jc / pocp), 1,400^2 (af); area is N x OWNED targets
    for m in ("gcs", "jc", "pocp"):
        assert pick(m, side=2199) == "popc" and pick(m, side=2200) == "sparsecol", m
        assert pick(m, n=2200, nown=2199) == "popc" and pick(m, n=4840, nown=1000) == "sparsecol" and pick(m, n=4839, nown=1000) == "popc", m
    assert pick("af", side=1399) == "sparse64" and pick("af", side=1400) == "sparsecol" and pick("af", n=1400, nown=1399) == "sparse64"
    # ... and its words: more than 40 + 8 x shared (2.5 shared: 60 exactly)
    for m in C.SET_METRICS:
        assert pick(m, words=60, avg_shared=2.5) != "sparsecol" and pick(m, words=61, avg_shared=2.5) == "sparsecol", m
        assert pick(m, words=61, avg_shared=2.625) != "sparsecol", m
    # ... and its masks: 7,872 phams with two holders (123 words of 64; 8 B each beside 16,640 B of accumulators in 78 KB); pocp / af
    # 6,272 (beside a value table of at least 1,024 entries: at 6,272 it holds 1,151)
    for m in ("gcs", "jc"):
        assert pick(m, two_holder=7872) == "sparsecol" and pick(m, two_holder=7873) == "popc", m
        assert pick(m, two_holder=7873, forced="sparsecol") == "popc", m
    for m in ("pocp", "af"):
        assert pick(m, two_holder=6272, max_block_entries=1151) == "sparsecol", m
        assert pick(m, two_holder=6272, max_block_entries=1152) == "sparse64", m              # (pocp: 3,000^2 >= 2,500^2 and 79 > 28 + 4.3 x 2.85)
        assert pick(m, two_holder=6273, max_block_entries=100) == "sparse64", m
    # the value table's cap at 5,056 mask entries: (81,664 - 5,056 x 10 - 16,640) / 2 - 1 = 7,231
    for m in ("pocp", "af"):
        assert pick(m, max_block_entries=7231) == "sparsecol" and pick(m, max_block_entries=7232) == "sparse64", m
        assert pick(m, max_block_entries=7232, forced="sparsecol") == "sparse64", m
    assert pick("pocp", max_block_entries=7232, side=2200) == "popc"                              # (below 2,500^2)
    assert pick("jc", max_block_entries=1 << 40) == "sparsecol"                                 # gcs / jc keep no values
    # 16-bit values: af's entry lengths, pocp's gene counts (two per register in sparse64 as well)
    assert pick("af", max_ent_len=65535) == "sparsecol" and pick("af", max_ent_len=65536) == "sparse64"
    assert pick("pocp", max_ent_len=65536) == "sparsecol" and pick("jc", max_ent_len=65536) == "sparsecol"
    assert pick("pocp", max_ngen=65535) == "sparsecol" and pick("pocp", max_ngen=65536) == "popc"
    assert pick("pocp", max_ngen=65535, two_holder=7873) == "sparse64" and pick("pocp", max_ngen=65536, two_holder=7873) == "popc"
    assert pick("pocp", max_ngen=65536, forced="sparse64") == "popc" and pick("pocp", max_ngen=65536, forced="sparsecol") == "popc"
    assert pick("af", max_ngen=65536) == "sparsecol" and pick("jc", max_ngen=65536) == "sparsecol"
    # af: "sum == 0" must mean "nothing shared" (no empty translation) and totals must fit 31 bits -- else 32 x 32 tiles up to 3,500^2, then the walker
    assert pick("af", min_gene_len=0, side=3500) == "sparse" and pick("af", min_gene_len=0, side=3501) == "walker"
    assert pick("af", min_gene_len=0, n=12250, nown=1000) == "sparse" and pick("af", min_gene_len=0, n=12251, nown=1000) == "walker"
    assert pick("af", max_tlen=(1 << 31) - 1) == "sparsecol" and pick("af", max_tlen=1 << 31) == "sparse"
    for forced in ("sparse64", "sparsecol"):
        assert pick("af", min_gene_len=0, forced=forced) == "sparse"
    assert pick("pocp", min_gene_len=0) == "sparsecol" and pick("gcs", min_gene_len=0) == "sparsecol"
    assert pick("jc", max_nph=(1 << 30) - 1) == "sparsecol" and pick("jc", max_nph=1 << 30) == "popc"
    # gcs / jc on sparse64 (masks beyond the column kernel): words > 113 + 5.4 x shared from 3,000^2, > 60 + 5.4 x shared from 6,000^2
    many = dict(two_holder=7873, avg_shared=0.0)
    for m in ("gcs", "jc"):
        assert pick(m, words=113, **many) == "popc" and pick(m, words=114, **many) == "sparse64" and pick(m, words=114, side=2999, **many) == "popc", m
        assert pick(m, words=126, two_holder=7873, avg_shared=2.5) == "popc" and pick(m, words=127, two_holder=7873, avg_shared=2.5) == "sparse64", m   # 113 + 13.5
        assert pick(m, words=61, side=6000, **many) == "sparse64" and pick(m, words=60, side=6000, **many) == "popc" and pick(m, words=61, side=5999, **many) == "popc", m
    # pocp on sparse64: words > 28 + 4.3 x shared from 2,500^2
    assert pick("pocp", words=28, side=2500, **many) == "popc" and pick("pocp", words=29, side=2500, **many) == "sparse64"
    assert pick("pocp", words=29, side=2499, **many) == "popc" and pick("pocp", words=37, side=2500, two_holder=7873, avg_shared=2.0) == "sparse64"      # 28 + 8.6
    assert pick("pocp", words=36, side=2500, two_holder=7873, avg_shared=2.0) == "popc"
    # af: sparse64 at every size below the column kernel's
    assert pick("af", side=2) == "sparse64" and pick("af", side=1399, words=5, avg_shared=34.0) == "sparse64" and pick("af", side=20000, words=5, avg_shared=34.0) == "sparse64"
    # a forced family is taken where it exists for the metric
    for m in C.SET_METRICS:
        counts = m in ("gcs", "jc")
        assert pick(m, forced="popc") == ("sparsecol" if m == "af" else "popc"), m
        assert pick(m, forced="sparse") == ("sparsecol" if counts else "sparse"), m
        assert pick(m, forced="walker") == ("sparsecol" if counts else "walker"), m
        assert pick(m, forced="sparse64") == "sparse64" and pick(m, forced="sparsecol", side=100) == "sparsecol", m
    lib = hip.load()
    assert lib.pc_set_kernel_choice(None) == -1 and lib.pc_last_set_launch(None, None, None) == -1                    # PC_ERR_ARG
    with pytest.raises(hip.HipLibraryError):
        C.set_kernel_choice("jc", **_choice_base(nown=3001))


def test_set_block_entries_counts_the_ragged_block(native_built):
    """max_block_entries of the selector's inputs: blocks of 64 consecutive OWNED targets, and the last block of a shard -- fewer
    than 64 targets -- counts: here it alone exceeds the value table, so the rank leaves the column kernel where the unsharded fill,
    whose blocks are cut elsewhere, stays."""
    import set_kernel_cases as S
    from phamclust_amd import hip
    C = hip.Context
    per = np.full(200, 100, dtype=np.int64)
    per[190:] = 2000                                                     # ten heavy genomes at the end
    owned = np.arange(100, 200)                                          # a rank's targets: blocks [100, 164) and the ragged [164, 200)
    assert C.set_max_block_entries(per, owned) == 26 * 100 + 10 * 2000 == 22600
    assert C.set_max_block_entries(per, owned[:64]) == 6400 and C.set_max_block_entries(per, owned[:65]) == 6400
    assert C.set_max_block_entries(per, np.arange(200)) == 8 * 2000 == 16000          # unsharded: [192, 200) is the last block
    assert C.set_max_block_entries(per, np.arange(0)) == 0
    assert C.set_max_block_entries(per, np.array([199, 0])) == 2100       # (owned[] is what it is given: no sorting, no dedup)
    stats = {"sp_n": per}
    assert int(S.block_entries(stats, owned).max()) == 22600 and S.block_entries(stats, owned).tolist() == [6400, 22600]
    assert int(S.block_entries(stats).max()) == 16000 and S.block_entries(stats).shape == (4,)
    # the numpy recount and the library agree on every shard of a designed collection
    packed, st = S.collection("few400_empty")
    costs = S.target_costs(packed)
    for world in (1, 3, 8):
        for balanced in S.DEALS:
            for rank in range(world):
                own = S.owned_targets(packed, rank, world, balanced, costs)
                assert C.set_max_block_entries(st["sp_n"], own) == S.selector_inputs(st, own)["max_block_entries"]
    # ragged block decides: cap 7,231 at 5,056 mask entries
    base = _choice_base(n=3000, nown=100)
    light, heavy = np.full(3000, 100), np.full(3000, 100)
    heavy[2990:] = 400                                                   # [2964, 3000) of a rank owning [2900, 3000): 26 x 100 + 10 x 400 = 6,600 ... no overflow
    assert C.set_max_block_entries(heavy, np.arange(2900, 3000)) == 6600
    heavy[2990:] = 500                                                   # 2,600 + 5,000 = 7,600 > 7,231
    n_ragged = C.set_max_block_entries(heavy, np.arange(2900, 3000))
    assert n_ragged == 7600 and C.set_max_block_entries(light, np.arange(2900, 3000)) == 6400
    base.update(n=30000, nown=100)                                       # (area 3,000,000 >= 1,400^2)
    assert C.set_kernel_choice("af", **dict(base, max_block_entries=6400)) == "sparsecol"
    assert C.set_kernel_choice("af", **dict(base, max_block_entries=n_ragged)) == "sparse64"


def test_set_launch_shape_pins(native_built):
    """pc_set_launch_shape on both sides of every threshold inside the five launchers, by hand from pc_set_shape.hip (256 compute units)."""
    from phamclust_amd import hip
    C = hip.Context

    def shape(family, metric, n, nown=None, words=79, two_holder=5000, **kw):
        return C.set_launch_shape(family, metric, n, n if nown is None else nown, words, two_holder, **kw)

    def edge(tiles_x, tiles_y, top=8):
        e = top
        while e > 1 and -(-tiles_x // e) * -(-tiles_y // e) < 128:
            e //= 2
        return e
    # popcount tiles: 64 x 64 from 1,536 live tiles (half of the 64-tiles); N = 3,520 / 3,521: 55^2 / 2 = 1,512, 56^2 / 2 = 1,568
    assert shape("popc", "jc", 3520)["tile"] == 32 and shape("popc", "jc", 3521)["tile"] == 64
    assert shape("popc", "pocp", 5312, 2368)["tile"] == 32 and shape("popc", "pocp", 4096, 3072)["tile"] == 64          # 83 x 37 = 3,071; 64 x 48 = 3,072
    assert shape("popc", "gcs", 3521, popc_tile=32)["tile"] == 32 and shape("popc", "gcs", 100, popc_tile=64)["tile"] == 64
    s = shape("popc", "jc", 3521)                                    # 56 x 56 tiles: edge 8 -> 49 super-tiles, 4 -> 196; 14 rows x 2 x 8 XCDs x 16
    assert (s["super_edge"], s["grid"], s["units"], s["units_per_wg"], s["lds"], s["chunks"]) == (4, 3584, 3584, 1, 0, 0)
    # super-tile edge: halved while fewer than 128 super-tiles -- 32-tiles: 22 / 23, 44 / 45, 88 / 89 tiles a side
    for n, e in ((704, 1), (705, 2), (1408, 2), (1409, 4), (2816, 4), (2817, 8)):
        for family, metric in (("popc", "jc"), ("sparse", "af"), ("walker", "pocp")):
            assert shape(family, metric, n, popc_tile=32)["super_edge"] == e, (family, n)
    assert shape("popc", "jc", 20000)["super_edge"] == 8 and shape("sparse64", "jc", 20000)["super_edge"] == 16
    for n, e in ((11264, 8), (11265, 16), (5632, 4), (5633, 8)):      # 64-tiles, top edge 16: 176 / 177 and 88 / 89 tiles a side
        assert shape("sparse64", "af", n)["super_edge"] == e, n
    assert shape("popc", "jc", 6400, 2134)["super_edge"] == 4 == edge(100, 34) and shape("popc", "jc", 6400, 2134)["grid"] == 9 * 4 * 8 * 16   # a trapezoid
    assert shape("walker", "af", 3600)["grid"] == shape("sparse", "af", 3600, words=19, two_holder=1200)["grid"] == 15 * 2 * 8 * 64     # 113 tiles: edge 8
    # 64 x 64 sparse tiles: one unit per workgroup up to 2,048 units (4 x the 512 resident workgroups), then about three
    s = shape("sparse64", "af", 4096, 2048, words=19, two_holder=1200)          # 64 x 32 tiles, edge 4: 8 rows x 2 x 8 x 16
    assert (s["super_edge"], s["units"], s["grid"], s["units_per_wg"]) == (4, 2048, 2048, 1)
    s = shape("sparse64", "af", 4096, 2049, words=19, two_holder=1200)          # 33 tile rows: 9 x 2 x 8 x 16
    assert (s["units"], s["grid"], s["units_per_wg"]) == (2304, 2048, 2)
    s = shape("sparse64", "af", 6000, words=19, two_holder=1200)
    assert (s["super_edge"], s["units"], s["grid"], s["units_per_wg"]) == (8, 12288, 4096, 3)
    assert shape("sparse64", "af", 6000, words=19, two_holder=1200, n_cu=64)["grid"] == 4096 and shape("sparse64", "af", 2560, n_cu=64)["grid"] == 640   # (4 x 128 resident < a third of 1,920 units)
    # ... mask chunks: one up to 7,680 entries (af's two-batch instance stages broadcasts: 6,912), two from 4,000 x 4,000 with 2,048 entries
    s = shape("sparse64", "jc", 100, two_holder=7680)
    assert (s["chunks"], s["chunk"], s["batches"], s["dense"], s["lds"]) == (1, 7680, 2, 0, 7680 * 8 + 16640)
    s = shape("sparse64", "jc", 100, two_holder=7681)
    assert (s["chunks"], s["chunk"], s["batches"], s["dense"], s["lds"]) == (2, 3904, 1, 0, 3904 * 8 + 16640)
    s = shape("sparse64", "af", 100, two_holder=6912)
    assert (s["chunks"], s["chunk"], s["batches"], s["dense"], s["lds"]) == (1, 6912, 2, 1, 6912 * 8 + 16640 + 6144)
    s = shape("sparse64", "af", 100, two_holder=6913)
    assert (s["chunks"], s["chunk"], s["batches"], s["dense"], s["lds"]) == (2, 3520, 1, 0, 3520 * 8 + 16640)
    assert shape("sparse64", "pocp", 100, two_holder=6913)["chunks"] == 1 and shape("sparse64", "pocp", 100, two_holder=7681)["chunks"] == 2
    for m in C.SET_METRICS:
        assert shape("sparse64", m, 4000, 3999)["chunks"] == 1 and shape("sparse64", m, 4000)["chunks"] == 2 and shape("sparse64", m, 4000)["chunk"] == 2560, m
        assert shape("sparse64", m, 4000, two_holder=1984)["chunks"] == 1 and shape("sparse64", m, 4000, two_holder=1985)["chunks"] == 2, m   # 31 / 32 words
        assert shape("sparse64", m, 4000)["batches"] == 1 and shape("sparse64", m, 4000)["dense"] == 0 and shape("sparse64", m, 4000, 3999)["dense"] == (m == "af"), m
    assert shape("sparse64", "jc", 100, s64_chunks=3)["chunks"] == 3 and shape("sparse64", "jc", 100, s64_chunks=3)["chunk"] == 27 * 64
    assert shape("sparse64", "jc", 100, two_holder=128, s64_chunks=3)["chunks"] == 1                       # (more chunks than words: ignored)
    # 32 x 32 sparse tiles: every pham of the VOCABULARY in one chunk up to 10,240, else 8,192 at a time
    s = shape("sparse", "af", 100, words=160)
    assert (s["chunks"], s["chunk"], s["lds"]) == (1, 10240, 10240 * 4 + 8192)
    s = shape("sparse", "pocp", 100, words=161)
    assert (s["chunks"], s["chunk"], s["lds"]) == (2, 8192, 8192 * 4 + 8192)
    # column kernel: seg = live tiles / (4 x 256), 1 ... 8; live = blocks x tiles / 2 + blocks
    s = shape("sparsecol", "jc", 4032)                               # 63: 1,984 + 63 = 2,047
    assert (s["seg"], s["runs"], s["grid"], s["lds"], s["vals_cap"], s["super_edge"]) == (1, 63, 64 * 65, 5056 * 8 + 16640, 0, 0)
    s = shape("sparsecol", "af", 4033)                               # 64: 2,048 + 64
    assert (s["seg"], s["runs"], s["grid"], s["lds"], s["vals_cap"]) == (2, 32, 64 * 34, 80 * 1024 - 256, 7231)
    s = shape("sparsecol", "pocp", 20000)
    assert (s["seg"], s["runs"], s["grid"]) == (8, 40, 320 * 42)
    assert shape("sparsecol", "jc", 7200, 2400)["seg"] == 2 and shape("sparsecol", "jc", 7200, 900)["seg"] == 1        # 38 x 113 / 2 + 38 = 2,185; 15 x 113 / 2 + 15 = 862
    assert shape("sparsecol", "jc", 20000, col_seg=1)["runs"] == 313 and shape("sparsecol", "jc", 20000, col_seg=64)["runs"] == 5
    assert shape("sparsecol", "jc", 20000, col_seg=65)["seg"] == 8 and shape("sparsecol", "jc", 4033, n_cu=64)["seg"] == 8
    assert shape("sparsecol", "jc", 100, two_holder=7872)["lds"] == 7872 * 8 + 16640 and shape("sparsecol", "jc", 100, two_holder=7873)["lds"] == 0
    assert shape("sparsecol", "af", 100, two_holder=6272)["vals_cap"] == 1151 and shape("sparsecol", "pocp", 100, two_holder=6273)["vals_cap"] == 0
    assert shape("sparsecol", "pocp", 100, two_holder=6273)["lds"] == 0
    # epilogue table of the popcount tiles: (top + 1)(2 top + 1) entries for gcs / jc, (2 top + 1)^2 for pocp, up to 4 Mi
    assert 1448 * 2895 <= 4 << 20 < 1449 * 2897 and 2047 ** 2 <= 4 << 20 < 2049 ** 2
    for m in ("gcs", "jc"):
        assert shape("popc", m, 100, table_top=1447)["table"] == 1 and shape("popc", m, 100, table_top=1448)["table"] == 0, m
    assert shape("popc", "pocp", 100, table_top=1023)["table"] == 1 and shape("popc", "pocp", 100, table_top=1024)["table"] == 0
    # nothing to launch; arguments that name no launch
    assert shape("sparse64", "af", 1)["grid"] == 0 and shape("popc", "jc", 100, 0)["grid"] == 0
    for family, metric in (("popc", "af"), ("sparse", "jc"), ("walker", "gcs")):
        with pytest.raises(hip.HipLibraryError):
            shape(family, metric, 100)
    assert ctypes.sizeof(hip.PcSetInputs) == 72 and ctypes.sizeof(hip.PcSetShape) == 64


# Coverage classes a default process can reach (tests/set_kernel_cases.py: reachable_classes) that no unforced fill of the GPU
# tests reaches, each with its reason.  Keys are `class_of` tuples: (family, metric group, tile edge, super-tile edge, several
# units per workgroup, mask chunks > 1, (batches, dense), epilogue table, sharded).
SET_CLASSES_UNREACHED = {}          # (none left: few20000 / many20000 shard three ways at super-tile edge 16)


def test_set_kernel_cases_reach_every_class(native_built):
    """The unforced fills of tests/test_gpu_set_kernels.py (CASES: every collection unsharded, and by every rank of its worlds
    under both deals) together with the existing synth(20000, 5000) and synth_real(1000) fills reach every coverage class a
    default process can reach -- the sweep of the library's two host functions over N, nown <= 20,000, the generators' word /
    pham / shared ranges, an empty translation and an overflowing block (reachable_classes) -- except the classes listed above.
    Families and shapes come from the numpy recount of each packed collection, never from a context.  Numeric edges that no
    generator produces (65,536 genes, 1,448 phams in one genome ...) are the pins' and the GPU module's own cases."""
    import set_kernel_cases as S
    from phamclust_amd import hip
    C = hip.Context
    reachable = S.reachable_classes(C)
    cases = {**S.CASES, **S.EXISTING_CASES}
    by_case = S.classes_by_case(C, cases)
    assert set(S.EXPECTED_WHOLE) == set(S.CASES) == set(S.COLLECTIONS) - set(S.EXISTING_CASES)
    reached = S.union_classes(by_case)
    listing = "\n".join(f"{S.class_name(c)}  <-  {reached.get(c, SET_CLASSES_UNREACHED.get(c, 'NOTHING'))}" for c in sorted(set(reachable) | set(reached), key=str))
    assert len(SET_CLASSES_UNREACHED) == 0 and set(SET_CLASSES_UNREACHED) <= set(reachable) and not set(SET_CLASSES_UNREACHED) & set(reached), listing
    missing = set(reachable) - set(reached) - set(SET_CLASSES_UNREACHED)
    assert not missing, "no case reaches: " + "; ".join(S.class_name(c) for c in sorted(missing, key=str)) + "\n" + listing
    # what the issue names: the trapezoid classes of the 64-tile kernels beyond super-tile edge 1, several units, seg > 1 on a shard
    sharded = [c for c in reached if c[-1]]
    assert {c[3] for c in sharded if c[0] == "popc" and c[2] == 64} >= {4, 8}
    assert {c[3] for c in sharded if c[0] == "sparse64"} >= {1, 2, 4, 8} and any(c[4] for c in sharded if c[0] == "sparse64")
    assert any(c[4] for c in sharded if c[0] == "sparsecol") and any(not c[4] for c in sharded if c[0] == "sparsecol")
    assert {c[0] for c in reached} == set(S.FAMILIES)
    # the check has teeth: without col7200 no shard runs the column kernel with seg > 1; without the uniform draws pocp never
    # runs sparse64's two-batch instance
    fewer = S.union_classes(by_case, without=("col7200",))
    assert set(reachable) - set(fewer) - set(SET_CLASSES_UNREACHED) and not any(c[4] and c[-1] for c in fewer if c[0] == "sparsecol")
    fewer = S.union_classes(by_case, without=("uniform",))
    assert any(c[:2] == ("sparse64", "pocp") and c[6] == (2, 0) for c in set(reachable) - set(fewer))


def set_edges_fixture():
    """{(metric, as_distance): condensed vector} of tests/golden/set_edges/ (written by the LIVE reference), after checking that the
    committed generator still rebuilds the input the reference was given."""
    import json
    import set_kernel_cases as S
    from conftest import GOLDEN, read_adjacency_condensed
    manifest = json.load(open(os.path.join(GOLDEN, "set_edges", "manifest.json")))
    genomes = S.edge_genomes()
    assert [g.name for g in genomes] == list(S.EDGE_NAMES) == sorted(S.EDGE_NAMES)
    assert S.edge_digest(genomes) == manifest["input_sha256"], "the generator no longer reproduces the fixture's input"
    assert sum(len(g) for g in genomes) == manifest["genes"] == 136022 and manifest["pairs"] == 36
    want = {}
    for metric in S.SET_METRICS:
        names, dist, diag = read_lower_triangle(os.path.join(GOLDEN, "set_edges", manifest["files"][metric]["distance_lower_triangle"]))
        assert names == list(S.EDGE_NAMES) and not diag.any()
        want[(metric, True)] = dist
        want[(metric, False)], _ = read_adjacency_condensed(os.path.join(GOLDEN, "set_edges", manifest["files"][metric]["similarity_adjacency"]), names)
    return want


def test_set_edges_fixture_holds_both_oracles(native_built):
    """The numeric-edge collection (65,535 / 65,536 copies of a pham, 1,447 / 1,448 phams, 1,023 / 1,024 genes, entries of
    65,535 / 65,536 residues, empty translations): the C oracle and the Python restatement of metrics.py:26-157 equal what the
    live reference wrote for all 36 pairs, distance and similarity -- and so does every sub-collection the GPU tests upload."""
    import set_kernel_cases as S
    from oracle import oracle as O
    want = set_edges_fixture()
    genomes = S.edge_genomes()
    packed = S.edge_packed("all")
    stats = S.recount(packed)
    assert (stats["max_ngen"], stats["max_nph"], stats["max_ent_len"], stats["min_gene_len"]) == (65536, 1448, 65536, 0)
    py = {"gcs": O.py_gcs, "jc": O.py_jc, "pocp": O.py_pocp, "af": O.py_af}
    for (metric, dist), w in want.items():
        assert np.isfinite(w).all() and np.array_equal(O.fill(packed, metric, dist), w), (metric, dist)
        restated = np.array([py[metric](genomes[a], genomes[b], as_distance=dist) for a in range(9) for b in range(a + 1, 9)])
        assert np.array_equal(restated, w), (metric, dist)
    assert len({float(x) for x in want[("pocp", True)]}) > 20                      # (a collection whose pairs have values to get wrong)
    for subset, keep in S.EDGE_SUBSETS.items():
        sub = S.edge_packed(subset)
        assert sub.names == list(keep)
        for (metric, dist), w in want.items():
            assert np.array_equal(O.fill(sub, metric, dist), S.sub_condensed(w, list(S.EDGE_NAMES), keep)), (subset, metric, dist)
    # which side of each guard the sub-collections sit on
    side = {name: S.recount(S.edge_packed(name)) for name in S.EDGE_SUBSETS}
    assert (side["lo"]["max_ngen"], side["lo"]["max_nph"], side["lo"]["max_ent_len"], side["lo"]["min_gene_len"]) == (65535, 1447, 65535, 1)
    assert (side["hi"]["max_ngen"], side["hi"]["max_nph"], side["hi"]["max_ent_len"], side["hi"]["min_gene_len"]) == (65536, 1448, 65536, 1)
    assert side["genes1023"]["max_ngen"] == 1023 and side["genes1024"]["max_ngen"] == 1024 and side["phams1447"]["max_nph"] == 1447
    assert side["phams1448"]["max_nph"] == 1448 and side["empty"]["min_gene_len"] == 0


def test_borrowed_array_guards_every_numpy_route():
    """a lent result must refuse ufuncs, reductions and numpy functions too once its loan has ended, not only
    indexing and conversion (host logic: the view class itself, over ordinary memory)."""
    from phamclust_amd import hip

    class Owner:
        pass
    base = np.arange(12, dtype=np.float64)
    lent = hip.BorrowedArray(base.view(), Owner())
    part = lent[2:5]                                          # a slice shares the loan
    assert lent.shape == (12,) and len(part) == 3 and lent.dtype == np.float64 and float(lent[3]) == 3.0
    assert type(np.asarray(lent)) is np.ndarray and np.array_equal(lent, base) and list(part) == [2.0, 3.0, 4.0]
    with pytest.raises(ValueError):
        lent[0] = 0.5
    assert float(np.sum(lent)) == 66.0 and type(lent + 1) is np.ndarray and (lent + 1)[0] == 1.0
    assert type(np.ascontiguousarray(lent)) is np.ndarray and np.concatenate([lent, part]).shape == (15,)
    assert float(part.max()) == 4.0 and float(np.dot(lent, lent)) == float(np.dot(base, base))
    into = np.zeros(12)
    np.add(lent, 1.0, out=into)
    assert into[3] == 4.0
    lent._end_loan()
    for use in (lambda: lent[0], lambda: lent.copy(), lambda: np.asarray(lent), lambda: np.sum(lent), lambda: lent + 1, lambda: lent.max(),
                lambda: np.ascontiguousarray(lent), lambda: np.concatenate([base, lent]), lambda: np.add(base, lent, out=into),
                lambda: part[0], lambda: part * 2.0, lambda: np.mean(part)):
        with pytest.raises(hip.HipLibraryError, match="loan has ended"):
            use()


def test_product_fails_loudly_without_library(monkeypatch, tmp_path):
    from phamclust_amd import hip
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", str(tmp_path / "missing.so"))
    with pytest.raises(hip.HipLibraryError):
        hip.load()
    with pytest.raises(hip.HipLibraryError):
        hip.Context(0)


def test_native_variant_selects_a_library_next_to_the_product_one():
    """PHAMCLUST_NATIVE_VARIANT=<name> (tools/build_variant.py: A/B of two builds in one GPU call) loads
    csrc/libphamclust_hip_<name>.so; unset -- or "asan", which names the HOST libraries' sanitized twins -- the product library;
    a variant that was never built fails loudly instead of falling back."""
    code = ("import os, sys; sys.path.insert(0, %r); from phamclust_amd import hip; print(os.path.basename(hip.LIB_PATH));\n"
            "try:\n    hip.load(); print('loaded')\nexcept hip.HipLibraryError: print('refused')") % REPO
    def run(variant):
        env = dict(os.environ)
        env.pop("PHAMCLUST_NATIVE_VARIANT", None)
        if variant is not None:
            env["PHAMCLUST_NATIVE_VARIANT"] = variant
        return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert run(None) == ["libphamclust_hip.so", "loaded"]
    assert run("asan")[0] == "libphamclust_hip.so"
    assert run("hooks")[0] == "libphamclust_hip_hooks.so"
    assert run("no_such_build") == ["libphamclust_hip_no_such_build.so", "refused"]


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under phamclust_amd/ may reference it."""
    pkg = os.path.join(REPO, "phamclust_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".c")):
                text = open(os.path.join(root, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "pc_oracle" not in text, f


def test_build_knows_every_unit_and_header():
    """The build's lists follow the sources: every csrc/*.hip is a unit of the HIP library (build.HIP_UNITS), and every csrc/*.h,
    with the public C-ABI header, is among the headers whose change makes an object stale."""
    from phamclust_amd import build
    on_disk = sorted(os.listdir(build.CSRC))
    units = {src for src, _, _ in build.HIP_UNITS}
    assert [f for f in on_disk if f.endswith(".hip") and f not in units] == []
    assert [u for u in units if u not in on_disk] == []
    stale_on = {os.path.realpath(h) for h in build.hip_headers()}
    assert [f for f in on_disk if f.endswith(".h") and os.path.realpath(os.path.join(build.CSRC, f)) not in stale_on] == []
    assert os.path.realpath(os.path.join(REPO, "include", "phamclust_hip.h")) in stale_on


def test_graft_entry_build(native_built):
    """The driver's build check (`__graft_entry__.build()`): compiles what is stale, imports the package, and
    agrees with the header about the ABI version."""
    import importlib
    import sys
    sys.path.insert(0, REPO)
    entry = importlib.import_module("__graft_entry__")
    entry.build()


def test_text_io_c_path_is_byte_identical(native_built, tmp_path):
    """The C row formatter / parser behind matrix_to_squareform, matrix_to_adjacency and read_squareform produce the
    bytes (and values) of the Python "%.6f" path, on rounded values and on arbitrary doubles (ties, tiny, 1.0)."""
    import ctypes
    from phamclust_amd import matrix as M
    lib = M._text_lib()
    assert lib is not None
    rng = np.random.default_rng(5)
    special = np.array([0.0, 1.0, 0.5, 1e-7, 4.9999999e-7, 5e-7, 5.0000001e-7, 0.9999995, 0.99999949, 0.1234565, 0.1234575,
                        2.5e-6, 3.5e-6, 123456.7890125, -0.0, -1e-9, -0.25, 1e8, 0.000001, 0.999999])
    values = np.concatenate([special, rng.random(5000), np.round(rng.random(5000), 6), rng.random(200) * 1e-6])
    cap = values.size * 24 + 1024
    buf = ctypes.create_string_buffer(cap)
    size = lib.pcp_format_row(values.ctypes.data, values.size, buf, cap)
    assert lib.pcp_format_row(values.ctypes.data, values.size, buf, 4000) == -1          # a buffer that cannot hold the row is refused, not overrun
    assert buf.raw[:size] == ("\t".join(f"{x:.6f}" for x in values.tolist()) + "\n").encode()
    back = np.empty(values.size)
    assert lib.pcp_parse_row(buf.raw[:size - 1], size - 1, back.ctypes.data, values.size) == values.size
    assert back.tolist() == [float(f"{x:.6f}") for x in values.tolist()]
    # whole files, both code paths
    n = 37
    names = [f"g{'x' * (i % 5)}{i:03d}" for i in range(n)]
    m = M.SymMatrix(names, is_distance=True)
    cond = np.round(rng.random(n * (n - 1) // 2), 6)
    cond[::7] = 0.0
    m = M.SymMatrix.from_condensed(names, cond, is_distance=True)
    outputs = {}
    for label, forced in (("c", lib), ("py", False)):
        M._TEXT_LIB = forced
        try:
            paths = [M.matrix_to_squareform(m, tmp_path / f"{label}_sq.tsv"), M.matrix_to_squareform(m, tmp_path / f"{label}_lt.tsv", lower_triangle=True),
                     M.matrix_to_adjacency(m, tmp_path / f"{label}_adj.tsv"), M.matrix_to_adjacency(m, tmp_path / f"{label}_adj0.tsv", skip_zero=True)]
            outputs[label] = [open(p, "rb").read() for p in paths]
            rows = [(name, row.tolist()) for name, row in M._read_rows(paths[1])]
            assert [r[0] for r in rows] == names and all(len(r[1]) == i + 1 for i, r in enumerate(rows))
            back = M.matrix_from_squareform(paths[1])
            outputs[label] += [rows, back.nodes, back.to_ndarray().tolist() if hasattr(back.to_ndarray(), "tolist") else back.to_ndarray()]
        finally:
            M._TEXT_LIB = lib
    assert outputs["c"] == outputs["py"]


def test_chunk_plan_arithmetic(native_built):
    """The rule by which a fill that exceeds its memory budget is cut into target ranges (pc_chunk_plan: host arithmetic in
    the library, no GPU).  Includes a plan of more than 2^31 alignments -- the size at which r02 refused ("shard the job"):
    every chunk stays below what one plan can index, the chunks tile the targets, and none is empty."""
    from phamclust_amd import hip
    rng = np.random.default_rng(5)
    assert hip.Context.chunk_plan([], 10).tolist() == [0]
    assert hip.Context.chunk_plan([5, 5, 5, 20, 1, 1, 1], 10).tolist() == [0, 2, 3, 4, 7]
    assert hip.Context.chunk_plan([0, 0, 0], 1).tolist() == [0, 3]
    assert hip.Context.chunk_plan([7], 1).tolist() == [0, 1]                   # one target above the budget: its own chunk
    # synth-like ramp: target t has ~2.7 alignments per pair (s, t), N = 60,000 genomes -> 4.9e9 alignments
    n = 60000
    counts = (np.arange(n, dtype=np.float64) * rng.uniform(1.5, 4.0, n)).astype(np.uint64)
    total = int(counts.sum())
    assert total > 2 ** 32
    limit = 2 ** 31 - 2
    cuts = hip.Context.chunk_plan(counts, limit)
    assert cuts[0] == 0 and cuts[-1] == n and (np.diff(cuts) > 0).all()
    sums = np.add.reduceat(counts, cuts[:-1])
    assert int(sums.sum()) == total and int(sums.max()) <= limit
    assert len(sums) <= total // limit + 2 + 1                                 # greedy: at most one chunk more than needed, +1 slack
    # a memory budget: 16 GiB of plan buffers at 56 B per alignment
    per_chunk = (16 << 30) // 56
    cuts = hip.Context.chunk_plan(counts, per_chunk)
    sums = np.add.reduceat(counts, cuts[:-1])
    assert int(sums.max()) <= per_chunk and len(sums) >= total // per_chunk
    # uint64 overflow of the running sum is a cut, not a wrap
    big = np.array([2 ** 63, 2 ** 63, 5], dtype=np.uint64)
    assert hip.Context.chunk_plan(big, 2 ** 64 - 1).tolist() == [0, 1, 3]


def test_gpus_request_is_clamped_to_the_work(native_built, tmp_path, monkeypatch):
    """`--gpus N` starts N ranks only when they can win back what starting them costs (the reference clamps its workers to
    the work as well, matrix.py:460-462).  The estimate is host arithmetic on the loaded genomes, before any GPU call; the
    log line says why the run stayed on one GPU."""
    from phamclust_amd import startup
    from phamclust_amd.synth import synth_packed
    small = synth_packed(120, 1500, seed=4)
    cells = startup.alignment_cells(small)
    from oracle import oracle as O
    _, n_aln, n_cells = O.fill_rows(small, "peq", 0, small.n_genomes)
    assert n_cells <= cells <= 1.2 * n_cells                       # an upper estimate, close (paralog-vs-paralog repeats only)
    n, why = startup.choose_gpus(8, small, "peq")
    assert n == 1 and "running on ONE GPU" in why and "8 GPUs" in why and "process group" in why
    assert startup.choose_gpus(1, small, "peq")[0] == 1
    assert startup.choose_gpus(4, small, "jc")[0] == 1             # set metrics: microseconds of kernel, never worth a launch
    monkeypatch.setenv("PHAMCLUST_LAUNCH_COST_S", "0.000001")
    n, why = startup.choose_gpus(8, small, "peq")
    assert n == 8 and "save up to" in why
    monkeypatch.delenv("PHAMCLUST_LAUNCH_COST_S")
    monkeypatch.setenv("PHAMCLUST_FORCE_GPUS", "1")                # what the launcher sets for the ranks it starts
    assert startup.choose_gpus(8, small, "peq")[0] == 8
    # a fill that does outweigh the start-up: cells scaled up by pretending every gene is 40 x longer
    monkeypatch.delenv("PHAMCLUST_FORCE_GPUS")
    import copy
    big = copy.copy(small)
    big.seq_off = small.seq_off * 40
    assert startup.estimate_fill_seconds(big, "peq") > 1600 * 0.9 * startup.estimate_fill_seconds(small, "peq") - 1.0
    # the in-process route (pc_multi_*) has almost nothing to start: the same request goes through once the fill is worth 0.35 s
    assert startup.multi_gpu_route() == "process"
    monkeypatch.setenv("PHAMCLUST_MULTI", "launcher")
    assert startup.multi_gpu_route() == "launcher"
    monkeypatch.delenv("PHAMCLUST_MULTI")
    assert startup.launch_cost_seconds(8, "process") < 0.1 * startup.launch_cost_seconds(8, "launcher") + 0.1
    n, why = startup.choose_gpus(8, small, "peq", route="process")
    assert n == 1 and "a context and an upload per device" in why          # 120 genomes: milliseconds of fill
    assert startup.choose_gpus(8, big, "peq", route="process")[0] == 8
    line = startup.Timeline()
    line.mark("imports")
    assert line.line().startswith("timing: {") and "imports" in line.as_dict()


def test_pipelined_strip_kernels_publish_after_their_stores():
    """the pipelined form of k_nw_strip hands boundary lines from wave to wave through HBM; the progress word that
    announces them must be stored after a vmcnt(0) wait (and, r05, with release / acquire atomics).  tools/check_pipe_publication.py
    compiles the alignment units to gfx950 assembly and checks every such kernel; a compiler update that reorders or drops the wait
    fails here, on the build machine, not as wrong scores on a GPU."""
    import subprocess
    import sys
    from conftest import REPO
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_pipe_publication.py")], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "8 pipelined strip kernels checked: ok" in run.stdout
