"""fp64 restatement of the ABX arithmetic, written from its description (not from either implementation): frame
distances, DTW with an explicit cost matrix and backtrack, and the per-triplet comparison counts.  Helper module of
tests/test_abx_*.py (not a test file); pinned to the reference by tests/test_abx_cpu.py against g19_abx.npz."""
import numpy as np


def frame_distances(x, y, distance):
    """[Lx, D] x [Ly, D] -> [Lx, Ly]: 'cosine' = acos(clamp(<x, y>, -1, 1)) / pi, 'euclidian' = ||x - y||."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if distance == "cosine":
        return np.arccos(np.clip(x @ y.T, -1.0, 1.0)) / np.pi
    return np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))


def dtw(d):
    """(cost / path length, path length) of the DTW over the distance matrix d: cost = d + min(up, diag, left); the
    length is that of the path traced back from the last cell, preferring diag, then left, then up on ties, and going
    straight along the first row / column once it reaches one."""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    cost = np.empty((n, m))
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                prev = 0.0
            elif i == 0:
                prev = cost[0, j - 1]
            elif j == 0:
                prev = cost[i - 1, 0]
            else:
                prev = min(cost[i - 1, j], cost[i - 1, j - 1], cost[i, j - 1])
            cost[i, j] = d[i, j] + prev
    i, j, length = n - 1, m - 1, 1
    while i > 0 and j > 0:
        up, left, diag = cost[i - 1, j], cost[i, j - 1], cost[i - 1, j - 1]
        if diag <= left and diag <= up:
            i, j = i - 1, j - 1
        elif left <= up:
            j -= 1
        else:
            i -= 1
        length += 1
    length += i + j
    return cost[n - 1, m - 1] / length, length


def dtw_margin(d):
    """(cost / path length, path length, margin): dtw's recursion and backtrack, plus how close the backtrack came to
    another path: the smallest (second smallest - smallest) / max(|second smallest|, 1e-30) among up, left and diag over
    the steps it took; inf when the path never leaves the first row or column.  A pair whose margin is above the relative
    error of an f32 running cost has the same path in f32.  (On lists of Python floats: the same fp64 operations as dtw,
    without numpy's per-element overhead.)"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    rows = d.tolist()
    cost = []
    for i in range(n):
        di = rows[i]
        ci = [0.0] * m
        if i == 0:
            prev = 0.0
            for j in range(m):
                prev = ci[j] = di[j] + prev
        else:
            up = cost[i - 1]
            ci[0] = di[0] + up[0]
            for j in range(1, m):
                ci[j] = di[j] + min(up[j], up[j - 1], ci[j - 1])
        cost.append(ci)
    i, j, length, margin = n - 1, m - 1, 1, np.inf
    while i > 0 and j > 0:
        up, left, diag = cost[i - 1][j], cost[i][j - 1], cost[i - 1][j - 1]
        lo, mid, _ = sorted((up, left, diag))
        margin = min(margin, (mid - lo) / max(abs(mid), 1e-30))
        if diag <= left and diag <= up:
            i, j = i - 1, j - 1
        elif left <= up:
            j -= 1
        else:
            i -= 1
        length += 1
    length += i + j
    return cost[n - 1][m - 1] / length, length, margin


def dtw_items(x, y, distance):
    return dtw(frame_distances(x, y, distance))


def group_dtw(xs, ys, distance, symmetric=False):
    """[len(xs), len(ys)] DTW matrix between lists of [L, D] items; symmetric: j > i computed as (x_i, y_j) and
    mirrored, diagonal NaN (excluded)."""
    out = np.full((len(xs), len(ys)), np.nan)
    for i in range(len(xs)):
        for j in range(i + 1 if symmetric else 0, len(ys)):
            out[i, j] = dtw_items(xs[i], ys[j], distance)[0]
            if symmetric:
                out[j, i] = out[i, j]
    return out


def counts(dxa, dxb):
    """(lt, eq, min gap): comparisons dxa[i, j] < dxb[i, k] and == over all (i, j, k) with dxa[i, j] not NaN, and the
    smallest |dxa - dxb| among them (how close a comparison came to flipping)."""
    a = dxa[:, :, None]
    b = dxb[:, None, :]
    ok = np.broadcast_to(~np.isnan(a), (dxa.shape[0], dxa.shape[1], dxb.shape[1]))
    lt = int(((a < b) & ok).sum())
    eq = int(((a == b) & ok).sum())
    gap = np.abs(a - b)[ok]
    return lt, eq, float(gap.min()) if gap.size else np.inf


def theta_band(dxa, dxb, n_norm, tol):
    """Interval of theta = (lt + eq / 2) / n_norm over every outcome of the comparisons whose gap is below tol."""
    a = dxa[:, :, None]
    b = dxb[:, None, :]
    ok = ~np.isnan(np.broadcast_to(a, (dxa.shape[0], dxa.shape[1], dxb.shape[1])))
    diff = (a - b)[ok]
    close = np.abs(diff) < tol
    sure_lt = ((diff < 0) & ~close).sum()
    n_close = close.sum()
    return sure_lt / n_norm, (sure_lt + n_close) / n_norm


def triplet_theta(a, b, x, distance, symmetric):
    """(theta, dxa, dxb) of one triplet of item lists, in fp64."""
    dxb = group_dtw(x, b, distance)
    dxa = group_dtw(x, a, distance, symmetric=symmetric)
    lt, eq, _ = counts(dxa, dxb)
    n_pos = len(a) * (len(a) - 1) if symmetric else len(a) * len(x)
    return (lt + 0.5 * eq) / (n_pos * len(b)), dxa, dxb
