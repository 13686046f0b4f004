#!/usr/bin/env python3
"""Generate tests/golden/nearest/ by running the LIVE reference's ``SymMatrix.nearest_neighbors`` (matrix.py:265-296).

Run where the reference is mounted only (as tests/golden/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nearest.py

The reference's own ``matrix_from_squareform`` reads the committed golden distance files (the lower triangles its
``matrix_to_squareform`` wrote), and its own ``nearest_neighbors(node, 1.0)`` -- the threshold wide open on distances -- ranks every
node's neighbours: closest first, equally close ones in node order.  Only what it returned is stored:

* ``small.json``      {metric: {node: [the 22 other names, nearest first]}} for the six metrics of the 23-genome collection
* ``synth200.json``   {"jc": {node: [the first 16 names]}} of the 200-genome collection

No reference code is imported into the package or copied here; nothing but name lists is written.
"""

import json
import os
import pathlib
import sys

HERE = pathlib.Path(__file__).resolve().parent
REFERENCE_SRC = "/root/reference/src"
SET_METRICS = ("gcs", "jc", "pocp", "af")


def rankings(matrix_from_squareform, path, cut=None):
    matrix = matrix_from_squareform(path)
    assert matrix.is_distance
    return {node: matrix.nearest_neighbors(node, 1.0)[:cut] for node in matrix.nodes}


def main():
    if not os.path.isdir(REFERENCE_SRC):
        sys.exit("the reference is not mounted here; fixtures are generated where it is")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REFERENCE_SRC)
    from phamclust.matrix import matrix_from_squareform          # the reference's reader and, behind it, its SymMatrix
    out_dir = HERE / "nearest"
    out_dir.mkdir(exist_ok=True)
    small = {}
    for metric in SET_METRICS + ("aai", "peq"):
        tag = "" if metric in SET_METRICS else ".oracle_nw"
        small[metric] = rankings(matrix_from_squareform, HERE / f"{metric}_distance_matrix{tag}.tsv")
    (out_dir / "small.json").write_text(json.dumps(small, separators=(",", ":")) + "\n")
    synth = {"jc": rankings(matrix_from_squareform, HERE / "synth200" / "jc_distance_matrix.tsv", cut=16)}
    (out_dir / "synth200.json").write_text(json.dumps(synth, separators=(",", ":")) + "\n")
    print("written:", *(f"{p.name} {p.stat().st_size} B" for p in sorted(out_dir.iterdir())))


if __name__ == "__main__":
    main()
