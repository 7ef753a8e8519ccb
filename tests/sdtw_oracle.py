"""Restatement of the subsequence DTW of query-by-example term detection, written from its definition (include/cpc2_hip.h,
DESIGN.md section 26) and not from the kernel.  Helper module of tests/test_term_detection_*.py (not a test file).

For a query of n frames and a document of m frames with frame distances d [n, m], every cell carries (cost, length, start):
row 0 has cost = d[0][j], length = 1, start = j; a cell of column 0 below it follows up; every other cell follows the
predecessor of smallest cost among diag, left and up (ties: diag, then left, then up); cost = d + pred.cost,
length = pred.length + 1, start = pred.start.  v[j] = cost[n-1][j] / length[n-1][j]; the score is min_j v[j], the first j
among equals; the outputs are score, start, end = j, length.

Clarity, carried forward: each cell also keeps the smallest and largest length and start over all predecessors whose cost is
within CLEAR relative of the smallest.  A pair is clear when the winning end column has one length and one start, and every
other column j has cost[j] / length_max[j] * (1 - CLEAR) > v_best * (1 + CLEAR): an f32 evaluation, whose running costs carry
a relative error of that scale, then finds the same integers."""
import math
from fractions import Fraction

import numpy as np

from tests.abx_oracle import frame_distances  # noqa: F401  (the frame distances are those of the ABX kernels)

CLEAR = 1e-5                      # the project's margin of an f32 running cost (tests/test_abx_scale_gpu.py)


def _cells(rows, n, m, track):
    """The last query row: lists cost, length, start (and lmin, lmax, smin, smax when track) over the columns."""
    cost = list(rows[0])
    length = [1] * m
    start = list(range(m))
    lmin, lmax, smin, smax = list(length), list(length), list(start), list(start)
    for i in range(1, n):
        di = rows[i]
        nc, nl, ns = [None] * m, [0] * m, [0] * m
        nlmin, nlmax, nsmin, nsmax = [0] * m, [0] * m, [0] * m, [0] * m
        for j in range(m):
            if j == 0:
                cands = ((cost[0], 0, False),)                      # (cost, column, in the new row): up only
            else:
                cands = ((cost[j - 1], j - 1, False), (nc[j - 1], j - 1, True), (cost[j], j, False))     # diag, left, up
            best = cands[0]
            for cand in cands[1:]:
                if cand[0] < best[0]:                               # strictly smaller only: ties stay with the earlier one
                    best = cand
            pc, pj, new = best
            nc[j] = di[j] + pc
            nl[j] = (nl[pj] if new else length[pj]) + 1
            ns[j] = ns[pj] if new else start[pj]
            if track:
                lo, hi, s_lo, s_hi = None, None, None, None
                bound = pc + CLEAR * abs(pc)
                for c, cj, cnew in cands:
                    if c <= bound:
                        a, b = (nlmin[cj], nlmax[cj]) if cnew else (lmin[cj], lmax[cj])
                        sa, sb = (nsmin[cj], nsmax[cj]) if cnew else (smin[cj], smax[cj])
                        lo = a if lo is None else min(lo, a)
                        hi = b if hi is None else max(hi, b)
                        s_lo = sa if s_lo is None else min(s_lo, sa)
                        s_hi = sb if s_hi is None else max(s_hi, sb)
                nlmin[j], nlmax[j], nsmin[j], nsmax[j] = lo + 1, hi + 1, s_lo, s_hi
        cost, length, start = nc, nl, ns
        lmin, lmax, smin, smax = nlmin, nlmax, nsmin, nsmax
    return cost, length, start, lmin, lmax, smin, smax


def sdtw(d):
    """(score, start, end, length, clear) of the distance matrix d [n, m], in float64."""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    cost, length, start, lmin, lmax, smin, smax = _cells(d.tolist(), n, m, True)
    v = [cost[j] / length[j] for j in range(m)]
    end = 0
    for j in range(1, m):
        if v[j] < v[end]:
            end = j
    clear = lmin[end] == lmax[end] and smin[end] == smax[end]
    for j in range(m):
        if j != end and not cost[j] / lmax[j] * (1 - CLEAR) > v[end] * (1 + CLEAR):
            clear = False
    return v[end], start[end], end, length[end], clear


def sdtw_f32(d):
    """(score, start, end, length): the same program with every cost, sum and quotient in np.float32, for inputs whose costs
    are exact."""
    d = np.asarray(d, dtype=np.float32)
    n, m = d.shape
    cost, length, start = _cells([list(row) for row in d], n, m, False)[:3]
    v = [cost[j] / np.float32(length[j]) for j in range(m)]
    assert all(type(x) is np.float32 for x in v)
    end = 0
    for j in range(1, m):
        if v[j] < v[end]:
            end = j
    return v[end], start[end], end, length[end]


# --------------------------------------------------------------------------- inputs and scores shared by the tests
def speech_like(rng, m, dim=16, n_proto=12, noise=0.1, protos=None):
    """m frames made of runs of 2..8 noisy copies of n_proto prototypes."""
    protos = rng.standard_normal((n_proto, dim)) if protos is None else protos
    ids = []
    while len(ids) < m:
        ids += [int(rng.integers(0, n_proto))] * int(rng.integers(2, 9))
    return protos[np.array(ids[:m])] + noise * rng.standard_normal((m, dim))


def planted_case(rng, n, m):
    """A document of m frames and a query cut from a random span of n frames of it, 15 % of its frames dropped, 0.05 noise
    added: (query, document, first frame, last frame of the span that is left)."""
    doc = speech_like(rng, m)
    o = int(rng.integers(0, m - n + 1))
    keep = np.sort(rng.choice(n, n - int(round(0.15 * n)), replace=False))
    query = doc[o + keep] + 0.05 * rng.standard_normal((len(keep), doc.shape[1]))
    return query, doc, o + int(keep[0]), o + int(keep[-1])


def unit_rows(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


PLANTED = [(n, m, draw) for n in (20, 64, 65, 129) for m in (130, 200, 300) for draw in range(3)]


def fraction_scores(score, pair_q, pair_doc, relevant, n_queries):
    """MAP, mean P@10, mean P@N, MRR as Fractions, from a plain sort per query; and the queries without a relevant candidate."""
    sums, n_scored, without = [Fraction(0)] * 4, 0, []
    for q in range(n_queries):
        pairs = [p for p in range(len(score)) if pair_q[p] == q]
        pairs.sort(key=lambda p: (math.isnan(score[p]), 0.0 if math.isnan(score[p]) else score[p], pair_doc[p]))
        hits = [k + 1 for k, p in enumerate(pairs) if relevant[p]]
        if not hits:
            without.append(q)
            continue
        n_scored += 1
        n_rel = len(hits)
        parts = (sum(Fraction(k + 1, r) for k, r in enumerate(hits)) / n_rel, Fraction(sum(r <= 10 for r in hits), 10),
                 Fraction(sum(r <= n_rel for r in hits), n_rel), Fraction(1, hits[0]))
        sums = [a + b for a, b in zip(sums, parts)]
    return [s / n_scored for s in sums], without
