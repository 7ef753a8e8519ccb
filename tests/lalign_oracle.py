"""Restatement of the local alignment of spoken term discovery, written from its definition (include/cpc2_hip.h, DESIGN.md
section 28) and not from the kernel.  Helper module of tests/test_term_discovery_*.py (not a test file).

For a row item of n frames and a column item of m frames with frame distances d [n, m], a threshold theta > 0 and a step penalty
gamma >= 0:  g = theta - d[i][j];  the candidates of cell (i, j) are diag H[i-1][j-1] (i > 0 and j > 0), left H[i][j-1] - gamma
(j > 0) and up H[i-1][j] - gamma (i > 0); the best is the largest, ties to diag, then left, then up.  No candidate, or best <= 0:
the cell opens a path (h = g, length 1, start (i, j)); otherwise h = g + best, length = pred.length + 1, start = pred.start.
h > 0: the cell holds (H = h, length, start); otherwise H = 0 and it carries nothing (a NaN distance closes the cell).  The result
is the cell of largest H, among equals the smallest i, then the smallest j: (H, (start_i, end_i, start_j, end_j, length)), or
(0, (-1,) * 5) when no cell is positive.

Clarity, carried forward.  Two numbers are NEAR when they differ by at most CLEAR * max(|a|, |b|, theta): CLEAR relative, with the
scale of one gain as the floor, which is what "within that margin of 0" means here.  (A cell's h is a sum of gains theta - d with d
a frame distance known to a few f32 ulps of its size; at the decisions that matter |g| and |best| are of the order of theta, so an
f32 evaluation is off by some 1e-7 * theta per step: the margin leaves two orders of magnitude.)  A cell is UNSURE when
  - it continues a predecessor that is unsure, or another candidate NEAR the best carries another (length, start) or is unsure;
  - its open / continue decision is near: some candidate is NEAR 0 without being an exact 0 of a sure closed cell;
  - its clamp decision is near: h is NEAR 0.
A pair is clear when the best cell is sure, no other cell's H is NEAR the best, and, where the best is itself NEAR 0 (or there is
none), no clamp decision anywhere was near."""
import numpy as np

from tests.abx_oracle import frame_distances  # noqa: F401  (the frame distances are those of the ABX kernels)
from tests.sdtw_oracle import CLEAR, speech_like, unit_rows  # noqa: F401

NONE = (-1, -1, -1, -1, -1)


def _run(rows, n, m, theta, gamma, zero, track):
    """The whole matrix: (best H, span) and, when track, whether the pair is clear.  Arithmetic is that of the entries' type."""
    floor = float(theta)

    def near(a, b):
        return abs(a - b) <= CLEAR * max(abs(a), abs(b), floor)

    prev = None                                   # the row above: lists of H, length, start, unsure
    best_h, best = zero, NONE
    best_unsure, clamp_near, positives = False, False, []
    for i in range(n):
        di = rows[i]
        h_row, l_row, s_row, u_row = [zero] * m, [0] * m, [None] * m, [False] * m
        for j in range(m):
            g = theta - di[j]
            cands = []                            # (value, length, start, unsure) in the order diag, left, up
            if i > 0 and j > 0:
                cands.append((prev[0][j - 1], prev[1][j - 1], prev[2][j - 1], prev[3][j - 1]))
            if j > 0:
                cands.append((h_row[j - 1] - gamma, l_row[j - 1], s_row[j - 1], u_row[j - 1]))
            if i > 0:
                cands.append((prev[0][j] - gamma, prev[1][j], prev[2][j], prev[3][j]))
            pick = None
            for cand in cands:
                if pick is None or cand[0] > pick[0]:      # strictly larger only: ties stay with the earlier one
                    pick = cand
            unsure = False
            if pick is None or pick[0] <= 0:
                h, length, start = g, 1, (i, j)
            else:
                h, length, start = g + pick[0], pick[1] + 1, pick[2]
                if track:
                    unsure = pick[3] or any(near(c[0], pick[0]) and (c[3] or (c[1], c[2]) != (pick[1], pick[2])) for c in cands)
            if track:
                if pick is not None and pick[0] > 0:
                    unsure = unsure or near(pick[0], 0.0)
                else:                                       # opened: sure unless a candidate near 0 could have been positive; the
                    for c in cands:                         # H = 0 of a sure closed cell is 0 in every evaluation
                        if near(c[0], 0.0) and not (c[0] == 0 and c[1] == 0 and not c[3]):
                            unsure = True
                if near(h, 0.0):                            # (a NaN is near nothing: it closes the cell in every evaluation)
                    unsure = clamp_near = True
            if h > 0:
                h_row[j], l_row[j], s_row[j], u_row[j] = h, length, start, unsure
                if track:
                    positives.append(h)
                if h > best_h:                              # strict: the smallest i, then the smallest j among equals
                    best_h, best, best_unsure = h, (start[0], i, start[1], j, length), unsure
            else:
                u_row[j] = unsure                           # closed: H = 0 and nothing carried but the doubt
        prev = (h_row, l_row, s_row, u_row)
    if not track:
        return best_h, best
    clear = not best_unsure
    if sum(1 for h in positives if near(h, best_h)) > (1 if best != NONE else 0):
        clear = False
    if near(best_h, 0.0) and clamp_near:
        clear = False
    return best_h, best, clear


def local_align(d, theta, gamma):
    """(score, (start_i, end_i, start_j, end_j, length), clear) of the distance matrix d [n, m], in float64."""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    return _run(d.tolist(), n, m, float(theta), float(gamma), 0.0, True)


def local_align_f32(d, theta, gamma):
    """(score, span): the same program with every difference, sum and comparison in np.float32, for inputs whose sums are exact."""
    d = np.asarray(d, dtype=np.float32)
    n, m = d.shape
    score, span = _run([list(row) for row in d], n, m, np.float32(theta), np.float32(gamma), np.float32(0), False)
    assert type(score) is np.float32
    return score, span


# --------------------------------------------------------------------------- inputs shared by the tests
PLANTED_SIZES = ((40, 70), (64, 64), (65, 130), (129, 200), (200, 129))
PLANTED = [(n, m, draw) for n, m in PLANTED_SIZES for draw in range(4)]
FRAGMENT = 30                      # frames of the shared fragment before 15 % of them are dropped on one side


def planted_pair(rng, n, m, fragment=FRAGMENT, dim=16):
    """Two otherwise unrelated speech-like items (prototypes of their own) of n and m frames that share a fragment: `fragment`
    frames of a third prototype set stand in the first item; the second holds a copy with 15 % of the frames dropped and 0.05
    noise added.  Returns (a, b, (first_i, last_i, first_j, last_j)): the frames of the fragment that both sides hold."""
    a = speech_like(rng, n, dim=dim)
    b = speech_like(rng, m, dim=dim)
    frag = speech_like(rng, fragment, dim=dim)
    oa = int(rng.integers(0, n - fragment + 1))
    keep = np.sort(rng.choice(fragment, fragment - int(round(0.15 * fragment)), replace=False))
    ob = int(rng.integers(0, m - len(keep) + 1))
    a[oa:oa + fragment] = frag
    b[ob:ob + len(keep)] = frag[keep] + 0.05 * rng.standard_normal((len(keep), dim))
    return a, b, (oa + int(keep[0]), oa + int(keep[-1]), ob, ob + len(keep) - 1)


def planted_theta(d, distance):
    """The threshold of the planted family: 0.25 for the cosine distance, half the median distance for the euclidian."""
    return 0.25 if distance == "cosine" else 0.5 * float(np.median(d))
