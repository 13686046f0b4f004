"""CPU tests of the oracle itself (no GPU): golden fixtures from the live reference,
the two aligner formulations, math-pinned known answers, Python's round()."""

import random

import numpy as np
import pytest

from conftest import ALL_METRICS, SET_METRICS, golden_file, read_adjacency_condensed, read_lower_triangle


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


def test_blosum62_checksums(O):
    L = O.lib()
    m = [[L.pco_blosum62(i, j) for j in range(24)] for i in range(24)]
    assert all(m[i][j] == m[j][i] for i in range(24) for j in range(24))
    assert [m[i][i] for i in range(24)] == [4, 5, 6, 6, 9, 5, 5, 6, 8, 4, 4, 5, 5, 6, 7, 4, 5, 11, 7, 4, 4, 4, -1, 1]
    assert sum(m[i][j] for i in range(20) for j in range(20)) == -426
    assert sum(map(sum, m)) == -726
    assert min(map(min, m)) == -4 and max(map(max, m)) == 11
    assert L.pco_map(ord("a")) == L.pco_map(ord("A")) == 0 and L.pco_map(ord("J")) == 23 == L.pco_map(ord("*"))


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_c_oracle_vs_golden(O, small_packed, metric):
    """gcs/jc/pocp/af fixtures are pure reference output; aai/peq fixtures are the reference's
    metrics.py driven by this oracle's aligner (class "oracle_nw")."""
    names, gold, diag = read_lower_triangle(golden_file(metric))
    assert names == small_packed.names and not diag.any()
    assert np.array_equal(O.fill(small_packed, metric, as_distance=True), gold)
    gsim, dsim = read_adjacency_condensed(golden_file(metric, "similarity"), names)
    assert (dsim == 1.0).all()
    assert np.array_equal(O.fill(small_packed, metric, as_distance=False), gsim)


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_c_oracle_vs_reference_written_synth200(O, synth200_packed, metric):
    """19,900 pairs per metric written by the LIVE reference (matrix_de_novo over metrics.py:26-253, matrix.py:432-497; the file
    is what scripts/phamclust.py:262 caches) for the first 200 genomes of configs[1]'s workload: gcs / jc / pocp must be equal,
    af / aai / peq within 1e-6 (north_star) -- they are in fact equal too.  aai / peq files are class "oracle_nw" (the reference's
    loop over this oracle's aligner; parasail is absent)."""
    from conftest import synth200_file
    names, gold, diag = read_lower_triangle(synth200_file(metric))
    assert names == synth200_packed.names and len(names) == 200 and gold.shape == (19900,) and not diag.any()
    got = O.fill(synth200_packed, metric, as_distance=True)
    if metric in ("gcs", "jc", "pocp"):
        assert np.array_equal(got, gold)
    else:
        assert np.max(np.abs(got - gold)) <= 1e-6
        assert np.array_equal(got, gold)                     # stronger than the contract, and true


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_python_restatement_vs_golden(O, small_genomes, metric):
    names, gold, _ = read_lower_triangle(golden_file(metric))
    f = O.PY_METRICS[metric]
    n = len(small_genomes)
    vals = [f(small_genomes[i], small_genomes[j], as_distance=True) for i in range(n) for j in range(i + 1, n)]
    assert np.array_equal(np.array(vals), gold)


def test_aligner_formulations_agree(O):
    rng = random.Random(1)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    for it in range(4000):
        alpha = aa[:3] if it % 3 == 0 else aa           # a 3-letter alphabet forces many co-optimal ties
        a = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 48)))
        b = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 48)))
        tb = O.nw_traceback(a, b)
        score, ident, diag = O.nw_stats(a, b)
        assert score == tb.score
        assert ident == tb.comp.count("|")
        assert len(tb.query) == len(tb.ref) == len(tb.comp) == len(a) + len(b) - diag
        assert tb.query.replace("-", "") == a and tb.ref.replace("-", "") == b


@pytest.mark.parametrize("rule", list(range(1, 16)))
def test_aligner_formulations_agree_under_every_tie_rule(O, rule):
    """The table + traceback walk and the one-pass statistics are two implementations of each tie rule; the
    multi-rule pass behind tools/tie_sensitivity.py is a third.  All must agree, and the score never moves."""
    rng = random.Random(50 + rule)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    try:
        for it in range(400):
            alpha = aa[:3] if it % 3 else aa
            a = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 40)))
            b = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 40)))
            O.set_tie_rule(0)
            score0 = O.nw_stats(a, b)[0]
            O.set_tie_rule(rule)
            tb = O.nw_traceback(a, b)
            score, ident, diag = O.nw_stats(a, b)
            assert score == tb.score == score0
            assert ident == tb.comp.count("|") and len(tb.query) == len(a) + len(b) - diag
            assert tb.query.replace("-", "") == a and tb.ref.replace("-", "") == b
    finally:
        O.set_tie_rule(0)


def test_tie_sensitivity_pass_equals_single_rule_paths(O):
    from phamclust_amd.synth import synth_packed
    packed = synth_packed(24, 120, seed=5)
    iu = np.triu_indices(packed.n_genomes, 1)
    aai, peq, counters = O.tie_sensitivity(packed, iu[0], iu[1])
    assert counters[0, 1] == 0 and (counters[:, 0] == counters[0, 0]).all()
    try:
        for rule in range(16):
            O.set_tie_rule(rule)
            assert np.array_equal(O.pairs(packed, "aai", iu[0], iu[1], as_distance=False), aai[:, rule])
            assert np.array_equal(O.pairs(packed, "peq", iu[0], iu[1], as_distance=False), peq[:, rule])
    finally:
        O.set_tie_rule(0)


def test_tie_sensitivity_report_is_committed_and_consistent():
    """tests/golden/tie_sensitivity.json (tools/tie_sensitivity.py): the bound DESIGN.md quotes."""
    import json
    with open(golden_file("gcs").replace("gcs_distance_matrix.tsv", "tie_sensitivity.json")) as fh:
        rep = json.load(fh)
    assert [d["name"] for d in rep["datasets"]] == ["tests/golden/small_input.tsv", "synth(2000,5000)"]
    for ds in rep["datasets"]:
        assert len(ds["rules"]) == 16 and ds["rules"][0]["alignments_changed_frac"] == 0.0
    worst = rep["worst_case_over_rules_1_to_7"]
    assert 0.0 < worst["alignments_changed_frac"] < 0.05 and worst["max_abs_d_peq"] < 1e-3


def _rules_matching(O, vectors):
    """Tie rules (0..15) under which the oracle reproduces every (n_ident, aln_len) of the given parasail vectors."""
    ok = []
    try:
        for rule in range(16):
            O.set_tie_rule(rule)
            good = True
            for v in vectors:
                _, ident, diag = O.nw_stats(v["a"], v["b"])
                if ident != v["n_ident"] or len(v["a"]) + len(v["b"]) - diag != v["aln_len"]:
                    good = False
                    break
            if good:
                ok.append(rule)
    finally:
        O.set_tie_rule(0)
    return ok


def test_parasail_vectors_select_the_default_rule(O):
    """Runs only where someone has generated tests/golden/parasail_vectors.json with real parasail
    (tests/golden/make_parasail_vectors.py; impossible in this image).  Vectors whose score leaves the int16 range
    are excluded: the reference accepts parasail's saturated garbage there (metrics.py:174), this build computes in
    32 bits (tests/test_gpu_parity.py::test_int16_saturation_threshold)."""
    import json
    import os
    path = os.path.join(os.path.dirname(golden_file("gcs")), "parasail_vectors.json")
    if not os.path.exists(path):
        pytest.skip("no parasail vectors committed (parasail is not installable here): aligner parity stays UNPINNED")
    vectors = [v for v in json.load(open(path))["vectors"] if not v.get("saturated") and abs(v["score"]) < 32000]
    assert len(vectors) >= 100
    for v in vectors[:50]:
        assert O.nw_stats(v["a"], v["b"])[0] == v["score"]            # the score does not depend on any tie rule
    matching = _rules_matching(O, vectors)
    assert matching, "no tie rule reproduces parasail: a rule beyond the three switches is wrong"
    assert 0 in matching, f"parasail follows rule(s) {matching}, not the default 0: set PC_TIE_RULE / PC_TIE_RULE_DEFAULT accordingly"


def test_parasail_live_cross_check(O):
    """Opportunistic: with parasail importable, compare directly."""
    parasail = pytest.importorskip("parasail")
    rng = random.Random(7)
    vectors = []
    for it in range(300):
        alpha = "AGS" if it % 2 else "ACDEFGHIKLMNPQRSTVWY"
        a = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 80)))
        b = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 80)))
        tb = parasail.nw_trace_diag_16(a, b, 11, 1, parasail.blosum62).get_traceback(mch="|", sim="+", neg=" ")
        vectors.append({"a": a, "b": b, "aln_len": len(tb.query), "n_ident": tb.comp.count("|")})
    assert 0 in _rules_matching(O, vectors)


def test_aligner_known_answers(O):
    """Math-pinned cases: any correct affine NW (11/1, BLOSUM62) must return these."""
    s = "MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQ"
    tb = O.nw_traceback(s, s)
    assert tb.comp == "|" * len(s) and tb.score == sum(O.lib().pco_blosum62(O.lib().pco_map(ord(c)), O.lib().pco_map(ord(c))) for c in s)
    # one substitution: (L-1)/L identity, no gaps
    t = s[:10] + "W" + s[11:]
    tb = O.nw_traceback(s, t)
    assert "-" not in tb.query + tb.ref and tb.comp.count("|") == len(s) - 1
    # a clean internal deletion of 3 residues in a long, otherwise identical pair: one gap run of 3
    long = (s * 3)
    cut = long[:40] + long[43:]
    tb = O.nw_traceback(long, cut)
    assert tb.ref.count("-") == 3 and tb.query.count("-") == 0 and "---" in tb.ref
    assert tb.comp.count("|") == len(cut)
    # single residues
    assert O.nw_stats("M", "M") == (5, 1, 1)
    assert O.nw_stats("M", "W")[1:] == (0, 1)
    # case-insensitive identity, non-alphabet bytes score as '*' but only equal bytes are identical
    assert O.nw_stats("mkv", "MKV")[1] == 3
    assert O.nw_stats("J", "O") == (1, 0, 1) and O.nw_stats("J", "J") == (1, 1, 1)
    # boundary gaps cost open + (k-1)*extend: "A" vs "AAAA" -> 4 - (11 + 2)
    assert O.nw_stats("A", "AAAA")[0] == 4 - 13


def test_unique_optimum_by_brute_force(O):
    """Short pairs whose optimal alignment is provably unique (exhaustive enumeration):
    tie-breaking cannot matter, so these pin the aligner independently of parasail."""
    L = O.lib()

    def score(x, y):
        return L.pco_blosum62(L.pco_map(ord(x)), L.pco_map(ord(y)))

    def enumerate_alignments(a, b):
        # all (ops) sequences over {M, I(gap in a), D(gap in b)}
        out = []

        def rec(i, j, ops):
            if i == len(a) and j == len(b):
                out.append("".join(ops)); return
            if i < len(a) and j < len(b):
                rec(i + 1, j + 1, ops + ["M"])
            if j < len(b):
                rec(i, j + 1, ops + ["I"])
            if i < len(a):
                rec(i + 1, j, ops + ["D"])
        rec(0, 0, [])
        return out

    def ops_score(a, b, ops):
        i = j = 0; tot = 0; prev = None
        for op in ops:
            if op == "M":
                tot += score(a[i], b[j]); i += 1; j += 1
            else:
                tot -= 1 if prev == op else 11
                if op == "I": j += 1
                else: i += 1
            prev = op
        return tot

    rng = random.Random(4)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    checked = 0
    for _ in range(300):
        a = "".join(rng.choice(aa) for _ in range(rng.randint(1, 6)))
        b = "".join(rng.choice(aa) for _ in range(rng.randint(1, 6)))
        scored = sorted(((ops_score(a, b, ops), ops) for ops in enumerate_alignments(a, b)), reverse=True)
        if len(scored) > 1 and scored[0][0] == scored[1][0]:
            continue                                   # co-optimal: not a pinned case
        best, ops = scored[0]
        sc, ident, diag = O.nw_stats(a, b)
        assert sc == best and diag == ops.count("M")
        i = j = 0; want_ident = 0
        for op in ops:
            if op == "M":
                want_ident += a[i] == b[j]; i += 1; j += 1
            elif op == "I": j += 1
            else: i += 1
        assert ident == want_ident
        checked += 1
    assert checked > 100


def test_round6_is_python_round(O):
    rng = random.Random(2)
    xs = [rng.random() for _ in range(50000)]
    xs += [(rng.randint(0, 999999) + 0.5) / 1e6 for _ in range(50000)]
    xs += [rng.randint(0, 2 ** 20) / 2 ** rng.randint(1, 24) % 1.0 for _ in range(50000)]
    xs += [rng.randint(0, 300) / rng.randint(301, 700) for _ in range(50000)]
    xs += [0.0, 1.0, 0.5, 1 / 128, 3 / 128, 1 / 640, 5e-7, 4.9999999e-7, 1e-300, 0.9999995]
    for x in xs:
        assert O.round6(x) == round(x, 6), x


def test_synth_c_vs_python_restatement(O):
    """Packed closed forms (C) == per-pair dict/set semantics (Python) on synthetic genomes."""
    from phamclust_amd import build
    build.build_synth()
    from phamclust_amd.pack import unpack_genomes
    from phamclust_amd.synth import synth_packed
    packed = synth_packed(14, 300, seed=5)
    genomes = unpack_genomes(packed)
    n = len(genomes)
    for metric in ALL_METRICS:
        for as_distance in (True, False):
            want = [O.PY_METRICS[metric](genomes[i], genomes[j], as_distance=as_distance)
                    for i in range(n) for j in range(i + 1, n)]
            assert np.array_equal(O.fill(packed, metric, as_distance=as_distance), np.array(want))


def test_fill_rows_is_a_prefix(O, small_packed):
    full = O.fill(small_packed, "peq")
    part, n_aln, n_cells = O.fill_rows(small_packed, "peq", 0, 5)
    n = small_packed.n_genomes
    k = sum(n - 1 - s for s in range(5))
    assert np.array_equal(part[:k], full[:k]) and n_aln > 0 and n_cells > n_aln


def test_bulk_fill_equals_pairwise_for_every_metric():
    """pco_fill (OpenMP over the condensed index) and pco_pair answer alike for all seven selectors, percent-positives
    (aai, ppos=True: metrics.py:218-220) included -- the bulk path once treated that one as peq."""
    import numpy as np
    from oracle import oracle as O
    from phamclust_amd.synth import synth_packed
    pk = synth_packed(11, 150, seed=5)
    n = pk.n_genomes
    for metric in ("gcs", "jc", "pocp", "af", "aai", "peq", "aai_ppos"):
        for as_distance in (True, False):
            f = O.fill(pk, metric, as_distance)
            want = np.array([O.pair(pk, metric, s, t, as_distance=as_distance) for s in range(n) for t in range(s + 1, n)])
            assert np.array_equal(f, want), (metric, as_distance)
    assert (O.fill(pk, "aai_ppos", False) >= O.fill(pk, "aai", False)).all()


def test_checker_refuses_to_answer_with_switched_conventions():
    """pco_set_gap / pco_set_compat are process-global; a stray call must not turn later comparisons into ones
    against another aligner.  The matrix entry points answer under the defaults, or inside the scoped switches, only."""
    from oracle import oracle as O
    from phamclust_amd.synth import synth_packed
    pk = synth_packed(6, 60, seed=2)
    base = O.fill(pk, "peq")
    with O.gap(12, 1):
        other = O.fill(pk, "peq")                               # on purpose: allowed
    assert np.array_equal(O.fill(pk, "peq"), base) and other.shape == base.shape
    with O.compat(case_sensitive=True):
        O.pairs(pk, "aai", [0], [1])
    O.set_gap(12, 1)                                            # a bare call leaves the library switched ...
    try:
        for call in (lambda: O.fill(pk, "peq"), lambda: O.pairs(pk, "aai", [0], [1]), lambda: O.pair(pk, "peq", 0, 1),
                     lambda: O.fill_rows(pk, "peq", 0, 2)):
            with pytest.raises(RuntimeError, match="left switched"):
                call()
    finally:
        O.set_gap()                                             # ... until the defaults are restored
    assert np.array_equal(O.fill(pk, "peq"), base)


def test_markstein_division_by_a_million(O):
    """The set-metric epilogue ends in k / 1e6 (round(x, 6), e.g. metrics.py:50-53); the device computes it as a multiply and two
    fused multiply-adds (csrc/pc_pairs.h: pc_div_million).  In plain C arithmetic: the same value as the division for EVERY k a
    similarity or distance can produce (k <= 2 * 10^6; checked to 2^22).  The device side of the same claim:
    tests/test_gpu_parity.py::test_round6_every_millionth."""
    assert O.div_million_mismatches(1 << 22) == 0
