"""Plain numpy statements the bounded nearest fill and its two kernels are held to (tests/test_nearest_bound_host.py,
tests/test_gpu_nearest_bound.py, tests/nearest_bound_driver.py): k-nearest lists of a square, the edge list under a bar per genome,
and the five-step rule of ``results.neighbors._bounded_peq_nearest`` over two dense squares.  Nothing here calls the library."""

import numpy as np

PREFILTER_SLACK = 2e-6


def nearest_of_square(square, k, as_distance):
    """``(nbr, val)`` [n, min(k, n - 1)] of a symmetric square: per row one lexsort over (index, value), the better value first."""
    square = np.asarray(square, dtype=np.float64)
    n = square.shape[0]
    kk = max(min(int(k), n - 1), 0)
    nbr, val = np.empty((n, kk), dtype=np.int32), np.empty((n, kk), dtype=np.float64)
    for g in range(n):
        others = np.concatenate([np.arange(g), np.arange(g + 1, n)])
        row = square[g, others]
        order = np.lexsort((others, row if as_distance else -row))[:kk]
        nbr[g], val[g] = others[order], row[order]
    return nbr, val


def nearest_of_pairs(n, src, tgt, val, k, as_distance):
    """``(nbr, val, count)`` of a pair list, stated entry by entry in plain Python: every pair a candidate of both its ends, sorted by
    (value, better first; other end), cut after ``min(k, n - 1)``, padded with -1 / NaN."""
    kk = max(min(int(k), n - 1), 0)
    held = [[] for _ in range(n)]
    for s, t, v in zip(np.asarray(src).tolist(), np.asarray(tgt).tolist(), np.asarray(val, dtype=np.float64).tolist()):
        held[s].append((v if as_distance else -v, t, v))
        held[t].append((v if as_distance else -v, s, v))
    nbr, out = np.full((n, kk), -1, dtype=np.int32), np.full((n, kk), np.nan, dtype=np.float64)
    for g in range(n):
        for j, (_, h, v) in enumerate(sorted(held[g], key=lambda e: (e[0], e[1]))[:kk]):
            nbr[g, j], out[g, j] = h, v
    return nbr, out, np.array([len(one) for one in held], dtype=np.int32)


def passes(values, bar, as_distance):
    return values <= bar if as_distance else values >= bar


def edges_under_bars(square, bars, as_distance):
    """``(src, tgt, val)`` of the pairs (s < t) whose value passes ``bars[s]`` or ``bars[t]``, sorted by t, then s."""
    square, bars = np.asarray(square, dtype=np.float64), np.asarray(bars, dtype=np.float64)
    t, s = np.tril_indices(square.shape[0], k=-1)                      # row-major over the lower triangle: by t, then s
    v = square[s, t]
    keep = passes(v, bars[s], as_distance) | passes(v, bars[t], as_distance)
    return s[keep].astype(np.int32), t[keep].astype(np.int32), v[keep]


def bounded_rule(af_sim, peq, k, as_distance):
    """The five steps over the dense squares ``af_sim`` (af similarities) and ``peq`` (peq values in the call's direction): a dict with
    ``seed`` (src, tgt), ``bar``, ``simbar``, ``candidates`` (src, tgt), ``n_candidates``, ``fallback`` and the lists ``nbr`` / ``val``
    built from the candidates alone (also where the route would fall back: the rule is exact there too)."""
    af_sim, peq = np.asarray(af_sim, dtype=np.float64), np.asarray(peq, dtype=np.float64)
    n = af_sim.shape[0]
    kk = max(min(int(k), n - 1), 0)
    a_nbr, _ = nearest_of_square(af_sim, kk, False)
    g, h = np.repeat(np.arange(n, dtype=np.int64), kk), a_nbr.reshape(-1).astype(np.int64)
    pair = np.unique(np.maximum(g, h) * n + np.minimum(g, h))
    s_src, s_tgt = pair % n, pair // n
    _, l_val, l_count = nearest_of_pairs(n, s_src, s_tgt, peq[s_src, s_tgt], kk, as_distance)
    assert (l_count >= kk).all()
    bar = l_val[:, kk - 1].copy()
    simbar = ((1.0 - bar) - PREFILTER_SLACK) if as_distance else bar
    c_src, c_tgt, _ = edges_under_bars(af_sim, simbar, False)
    n_cand = int(c_src.shape[0])
    out = dict(seed=(s_src, s_tgt), bar=bar, simbar=simbar, candidates=(c_src, c_tgt), n_candidates=n_cand,
               fallback=2 * n_cand > n * (n - 1) // 2)
    out["nbr"], out["val"], count = nearest_of_pairs(n, c_src, c_tgt, peq[c_src, c_tgt], kk, as_distance)
    assert (count >= kk).all()
    return out
