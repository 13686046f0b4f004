"""The designed collection of tests/test_gpu_planner.py and the host-side arithmetic around it (no GPU call here).

A *case* is one bucket the device planner has to cut: ``(lb, rows, any_byte)`` -- a column sequence of ``lb`` residues
(``any_byte``: it holds a byte outside the 24-letter alphabet) with ``rows`` distinct row sequences.  `design` chooses the cases
from what the library's host functions say (`Context.bucket_launch_classes`, `Context.task_shape`), never by hand;
tests/test_host.py asserts on the CPU that they reach every launch class a default process can reach; `build` turns them into
genomes; `count` recounts alignments, cells and buckets from the packed arrays alone, by the reference's anchor rule
(metrics.py:204-217); `predict` turns buckets into tasks per launch class through the host cut.

Layout of the collection: source genomes (names sort first) and target genomes (names sort last).  A case of ``rows`` rows is
``rows`` phams, each held by its target (the SAME gene sequence of ``lb`` residues every time) and by exactly one source (a
distinct short gene).  Both hold one gene of the pham, so the later genome's gene -- the target's -- is the column
(pc_walk.hip, pc_visit) and the column sequence's bucket is the case's distinct rows.  No two sources and no two targets
share a case's pham: a bucket of n rows costs n alignments, not n^2 / 2.
"""

import numpy as np

ALPHABET = b"ARNDCQEGHILKMFPSTWYVBZX*"          # the 24 letters of the substitution table (either case)
COMMON = "ACDEFGHIKLMNPQRSTVWY"
OTHER = "UOJ0123456789"                          # bytes outside the alphabet
MAX_LB = 4096                                    # widest systolic variant: 64 lanes x 64 columns
MAX_ROWS = 2 * 208 + 16                          # two full tasks of the largest size and a wave round more
N_TARGETS, N_SOURCES = 9, 4
WINDOW_ROWS = (31, 32, 33, 64, 65)               # row lengths around the kernels' 32- and 64-entry staging windows
LONG_ROW = 1500


def base_class(C, lb, any_byte=False):
    return C.bucket_launch_classes(lb, 1, any_byte)["full"] // C.WAVE_MODES


def edge_lengths(C):
    """Column lengths on both sides of every change of base class (variant or lanes-per-segment bucket) up to MAX_LB."""
    lengths, prev = {1, MAX_LB}, base_class(C, 1)
    for lb in range(2, MAX_LB + 1):
        b = base_class(C, lb)
        if b != prev:
            lengths |= {lb - 1, lb}
        prev = b
    return sorted(lengths)


def strip_lengths(C):
    """For each wide variant the chooser gives a gene beyond MAX_LB residues (up to the 65,535 an upload accepts): the
    first such length.  {columns per lane: length}"""
    found = {}
    for lb in range(MAX_LB + 1, 65536, 1024):          # the chooser's cost changes with the pass count: every 1,024 residues at most
        found.setdefault(C.variant_width(lb), lb)
    return found


def bucket_sizes(C, lb, any_byte):
    """Row counts that give one row, nseg, nseg + 1, 2 nseg, 2 nseg + 1, every remainder the chooser moves and one it keeps,
    a full task exactly, one row more, and more than two tasks."""
    nseg = C.task_shape(lb)["streams"]
    per = C.bucket_launch_classes(lb, 1, any_byte)["per"]
    sizes, kept = {1, nseg, nseg + 1, 2 * nseg, 2 * nseg + 1, per, per + 1, 2 * per + 1}, False
    for r in range(1, nseg):
        moved = C.bucket_launch_classes(lb, nseg + r, any_byte)["rem"] >= 0
        if moved or not kept:
            sizes.add(nseg + r)
        kept = kept or not moved
    return sorted(sizes)


def design(C, lengths=None):
    """[(lb, rows, any_byte)] -- systolic cases at every edge length, then the strip-mined ones."""
    cases = []
    for lb in (edge_lengths(C) if lengths is None else lengths):
        for any_byte in (False, True):
            cases += [(lb, n, any_byte) for n in bucket_sizes(C, lb, any_byte)]
    for lb in strip_lengths(C).values():
        for any_byte in (False, True):
            cases += [(lb, n, any_byte) for n in bucket_sizes(C, lb, any_byte)]
    return cases


def classes_of(C, cases):
    """{launch class: first case that reaches it}"""
    reached = {}
    for case in cases:
        for cls in C.bucket_tasks(*case):
            reached.setdefault(cls, case)
    return reached


def class_name(C, cls):
    """'W=11 lanes<=64 any-byte one-wave' for a launch class id (for assertion messages)."""
    widths = sorted({C.variant_width(lb) for lb in range(1, MAX_LB + 1)})
    nvar = len(widths)
    base, mode = divmod(cls, C.WAVE_MODES)
    mode = ("own workgroup", "two waves", "one wave")[mode]
    if base >= nvar * 8 + 3:
        return f"general kernel, {mode}"
    if base >= nvar * 8:
        return f"strip-mined W={widths[nvar - 3 + base - nvar * 8]}, {mode}"
    any_byte, base = divmod(base, nvar * 4)
    return f"W={widths[base // 4]} lanes<={8 << (base % 4)}{' any-byte' if any_byte else ''}, {mode}"


# ---- the genomes ------------------------------------------------------------------------------------------------
def _letters(rng, n, alphabet=COMMON):
    return "".join(np.array(list(alphabet))[rng.integers(0, len(alphabet), n)])


def _row_lengths(rng, k, n, lb):
    """Mostly short; from 8 rows on a few around the staging windows and one long row, so that the row streams of a task
    are out of step; smaller buckets take one of those in turn.  Columns beyond 8,191 residues keep to short rows (their
    percent-positives run is the general kernel: one lane per alignment)."""
    lens = rng.integers(2, 25, n)
    special = list(WINDOW_ROWS) + ([LONG_ROW + int(rng.integers(0, 200))] if lb <= 8191 else [])
    if n >= 8:
        lens[rng.choice(n, len(special), replace=False)] = special
    elif n >= 2:
        lens[int(rng.integers(0, n))] = special[k % len(special)]
    return lens


def build(cases, seed=2026):
    """Name-sorted list[Genome] of the collection (deterministic)."""
    from phamclust_amd.genome import Genome
    rng = np.random.default_rng(seed)
    sources = [Genome(f"a_source_{i}") for i in range(N_SOURCES)]
    targets = [Genome(f"z_target_{i}") for i in range(N_TARGETS)]
    used_columns = set()
    for k, (lb, n, any_byte) in enumerate(cases):
        while True:                                     # a column sequence of its own per case: its bucket is this case's rows
            col = _letters(rng, lb)
            if any_byte:
                at = int(rng.integers(0, lb))
                col = col[:at] + OTHER[int(rng.integers(0, len(OTHER)))] + col[at + 1:]
            if col not in used_columns:
                break
        used_columns.add(col)
        rows, seen = [], set()
        for length in _row_lengths(rng, k, n, lb).tolist():
            while True:
                row = _letters(rng, length)
                if rng.random() < 0.03:                 # rows that hold bytes outside the alphabet, against any column
                    at = int(rng.integers(0, length))
                    row = row[:at] + OTHER[int(rng.integers(0, len(OTHER)))] + row[at + 1:]
                if row not in seen:
                    break
            seen.add(row)
            rows.append(row)
        target = targets[k % N_TARGETS]
        for i, row in enumerate(rows):
            sources[(i + k) % N_SOURCES].add(f"c{k:05d}_{i:03d}", row)
            target.add(f"c{k:05d}_{i:03d}", col)
        if k % 5 == 0:                                  # an alias: the same (row, column) pair once more, through another source
            sources[(k + 1) % N_SOURCES].add(f"c{k:05d}_alias", rows[0])
            target.add(f"c{k:05d}_alias", col)
    # paralogs on both sides, more on the source side: the anchor swaps to the target (its genes become the rows)
    for i in range(3):
        sources[0].add("x_swap", _letters(rng, 40 + 7 * i))
    for i in range(2):
        targets[0].add("x_swap", _letters(rng, 300 + 50 * i))
    for i in range(2):                                  # as many on both sides: the source stays the anchor
        sources[1].add("x_even", _letters(rng, 50 + i))
        targets[1].add("x_even", _letters(rng, 90 + i))
    # two paralogs with the same identity fraction (8 / 16 and 4 / 8) and different lengths: the tie goes to the last
    row = "ACDEFGHI"
    sources[2].add("x_tie", row)
    targets[2].add("x_tie", row + "WWWWWWWW"); targets[2].add("x_tie", "ACDEWYWY")
    sources[3].add("x_tie2", row)
    targets[3].add("x_tie2", "ACDEWYWY"); targets[3].add("x_tie2", row + "WWWWWWWW")
    # a pham every genome holds: source-source and target-target pairs, byte-identical genes among them
    shared = [_letters(rng, 60 + i) for i in range(5)]
    for i, g in enumerate(sources + targets):
        g.add("x_all", shared[i % len(shared)])
    return sorted(sources + targets, key=lambda g: g.name)


# ---- an independent count over the packed arrays ------------------------------------------------------------------
def count(packed):
    """What an aai / peq fill of `packed` must align, from the arrays alone: per pair of genomes and shared pham the genome
    with fewer genes of the pham is the anchor (tie: the first), every anchor gene is a row against every gene of the other
    (metrics.py:204-217); distinct alignments are distinct (row bytes, column bytes); a column's bucket is its distinct rows."""
    gene_off, seq_off = packed.gene_off, packed.seq_off
    blob = packed.residues.tobytes()
    seq_id, gene_seq, seq_len, seq_odd = {}, [], [], []
    upper = bytes(range(256)).upper()
    for g in range(packed.n_genes):
        raw = blob[seq_off[g]:seq_off[g + 1]]
        sid = seq_id.get(raw)
        if sid is None:
            sid = seq_id[raw] = len(seq_len)
            seq_len.append(len(raw))
            seq_odd.append(bool(raw.translate(upper).translate(None, ALPHABET)))
        gene_seq.append(sid)
    holders = {}
    genome_of = np.repeat(np.arange(packed.n_genomes), np.diff(gene_off)).tolist()
    for g, (genome, pham) in enumerate(zip(genome_of, packed.gene_pham.tolist())):
        holders.setdefault(pham, {}).setdefault(genome, []).append(g)
    n_cells = 0
    aln_row, aln_col, aln_target, aln_genes = [], [], [], []        # one entry per alignment: row / column sequence, target genome, (row gene, column gene)
    for by_genome in holders.values():
        if len(by_genome) < 2:
            continue
        order = sorted(by_genome)
        for i, s in enumerate(order):
            for t in order[i + 1:]:
                anchor, other = by_genome[s], by_genome[t]
                if len(anchor) > len(other):
                    anchor, other = other, anchor
                for a in anchor:
                    for b in other:
                        n_cells += seq_len[gene_seq[a]] * seq_len[gene_seq[b]]
                        aln_row.append(gene_seq[a]); aln_col.append(gene_seq[b]); aln_target.append(t); aln_genes.append((a, b))
    seq_len, seq_odd = np.array(seq_len, dtype=np.int64), np.array(seq_odd, dtype=bool)
    aln_row, aln_col, aln_target = (np.array(x, dtype=np.int64) for x in (aln_row, aln_col, aln_target))
    ct = {"n_alignments": len(aln_row), "n_cells": n_cells, "seq_len": seq_len, "seq_odd": seq_odd,
          "aln_row": aln_row, "aln_col": aln_col, "aln_target": aln_target,
          "per_target": np.bincount(aln_target, minlength=packed.n_genomes).astype(np.uint64)}
    key, first = np.unique(aln_col * len(seq_len) + aln_row, return_index=True)      # distinct (row, column), by column
    col = key // len(seq_len)
    ct["n_distinct_alignments"] = len(key)
    ct["n_distinct_cells"] = int((seq_len[key % len(seq_len)] * seq_len[col]).sum())
    genes = np.array(aln_genes, dtype=np.int32).reshape(-1, 2)[first]
    column_gene = {}                                     # ONE gene per column sequence: pc_align_pairs buckets rows by column gene
    for c, g in zip(col.tolist(), genes[:, 1].tolist()):
        column_gene.setdefault(c, g)
    ct["row_gene"] = genes[:, 0].copy()
    ct["column_gene"] = np.array([column_gene[c] for c in col.tolist()], dtype=np.int32)
    ct["buckets"] = buckets_by_group(ct, np.zeros(packed.n_genomes, dtype=np.int64))[0]
    return ct


def buckets_by_group(ct, group_of_target):
    """{group: sorted [(lb, rows, any_byte)]} when the target genomes are planned group by group (a chunk of a fill, a rank's
    shard): duplicates merge inside a group only.  group_of_target[t] < 0: nobody plans target t."""
    group = np.asarray(group_of_target, dtype=np.int64)[ct["aln_target"]]
    keep = group >= 0
    S = len(ct["seq_len"])
    key = np.unique((group[keep] * S + ct["aln_col"][keep]) * S + ct["aln_row"][keep])
    bucket, rows = np.unique(key // S, return_counts=True)           # (group, column sequence)
    out = {}
    for g, c, n in zip((bucket // S).tolist(), (bucket % S).tolist(), rows.tolist()):
        out.setdefault(g, []).append((int(ct["seq_len"][c]), n, bool(ct["seq_odd"][c])))
    return {g: sorted(v) for g, v in out.items()}


def predict(C, buckets, n_classes):
    """Tasks per launch class of those buckets by the host cut."""
    tasks = np.zeros(n_classes, dtype=np.int64)
    for lb, n, any_byte in buckets:
        for cls, k in C.bucket_tasks(lb, n, any_byte).items():
            tasks[cls] += k
    return tasks
