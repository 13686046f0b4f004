"""The child process of tests/test_gpu_nearest_bound.py: ``python nearest_bound_driver.py <case>`` under PHAMCLUST_NATIVE_VARIANT=hooks
and PHAMCLUST_NO_TORCH=1, as tests/slab_values_driver.py (the variant is chosen when phamclust_amd.hip is imported).

``bars_chunk_edges`` holds pc_fill_edges_bars to the numpy predicate on injected value triangles whose passing elements sit at the
first and the last slot of a chunk of the pass and on either side of every chunk edge; the chunk size is the library's
(``Context.rows_pass_span("edges")``).  It asserts everything itself and ends with ``ok <case> <number of comparisons>``."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import nearest_bound_cases as NB                                            # noqa: E402
import slab_value_cases as cases                                            # noqa: E402
from phamclust_amd import hip                                                # noqa: E402

METRIC = "jc"
COMPARED = [0]


def same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float64:
        got, want = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    assert np.array_equal(got, want), (label, int((got != want).sum()))
    COMPARED[0] += 1


def disjoint(n):
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:04d}")
        g.add(f"p{k}", "MKTAYIAKQRQISFVK")
        genomes.append(g)
    return pack_genomes(genomes)


def check(ctx, values, n, bars, as_distance, label, slabs):
    want = NB.edges_under_bars(cases.square(values, n), bars, as_distance)
    for slab_bytes in slabs:
        got = ctx.fill_edges_bars(METRIC, bars, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
        for arr, stated, what in zip(got[:3], want, ("src", "tgt", "val")):
            same(arr, stated, (label, what, as_distance, slab_bytes))
        assert got[3]["n_edges"] == want[0].shape[0], (label, got[3]["n_edges"])
    return want


def case_bars_chunk_edges():
    chunk = hip.Context.rows_pass_span("edges")
    n = 2
    while cases.n_pairs(n) < 2 * chunk + 2:                                  # two whole chunks and a ragged third
        n += 1
    pairs = cases.n_pairs(n)
    assert chunk >= 2 and 2 * chunk < pairs < 3 * chunk
    three = 8 * (pairs // 3 + n)
    assert len(hip.Context.edge_slabs(n, three)) - 1 == 3
    marked = [0, 1, chunk - 2, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, pairs - 1]
    s_of, t_of = cases.pair_ends(n)
    rng = np.random.default_rng(23)
    with hip.Context(0) as ctx:
        ctx.upload(disjoint(n), residues=False)
        for as_distance in (True, False):
            good, poor = (0.25, 0.75) if as_distance else (0.75, 0.25)
            nothing, everything = (-np.inf, np.inf) if as_distance else (np.inf, -np.inf)
            # only the marked elements pass, under one bar for all: exactly those come out, in order
            values = np.full(pairs, poor)
            values[marked] = good
            hip.set_slab_values(values)
            want = check(ctx, values, n, np.full(n, 0.5), as_distance, "marked, one bar", (0, three))
            assert want[0].tolist() == s_of[marked].tolist() and want[1].tolist() == t_of[marked].tolist()
            # each marked element alone, admitted by its source's bar, then by its target's
            for at in marked:
                for end in (s_of[at], t_of[at]):
                    bars = np.full(n, nothing)
                    bars[end] = 0.5
                    want = check(ctx, values, n, bars, as_distance, ("marked", at, int(end)), (0,))
                    assert (int(s_of[at]), int(t_of[at])) in set(zip(want[0].tolist(), want[1].tolist()))
            # every element passes the bar of the genomes at the marked elements' ends alone
            values = np.full(pairs, good)
            hip.set_slab_values(values)
            bars = np.full(n, nothing)
            bars[np.unique(np.concatenate([s_of[marked], t_of[marked]]))] = 0.5
            check(ctx, values, n, bars, as_distance, "open genomes", (0, three))
            # all different values, random bars among them with both infinities
            values = cases.ramp(n)
            hip.set_slab_values(values)
            for round_ in range(3):
                bars = rng.choice(values, n)
                bars[rng.random(n) < 0.2] = nothing
                bars[rng.random(n) < 0.05] = everything
                check(ctx, values, n, bars, as_distance, ("ramp", round_), (0, three))
            hip.set_slab_values(None)
        # equal bars on injected values: the threshold fill's list
        values = cases.tie_set(n, 29)
        hip.set_slab_values(values)
        for as_distance in (True, False):
            for got, want in zip(ctx.fill_edges_bars(METRIC, np.full(n, 0.5), as_distance=as_distance, slab_bytes=three),
                                 ctx.fill_edges(METRIC, 0.5, as_distance=as_distance)):
                same(got, want, ("equal bars", as_distance))
        hip.set_slab_values(None)


CASES = {"bars_chunk_edges": case_bars_chunk_edges}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print("usage: nearest_bound_driver.py <" + " | ".join(CASES) + ">")
        return 2
    assert os.environ.get("PHAMCLUST_NATIVE_VARIANT") == "hooks" and hip.load().pc_test_hooks() == 1, "not the test-hooks twin of the library"
    CASES[argv[1]]()
    assert hip._slab_values is None, "a case left the hook set"
    print(f"ok {argv[1]} {COMPARED[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
