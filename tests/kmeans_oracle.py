"""fp64 numpy oracle of the k-means arithmetic (cpc/clustering/clustering.py of the reference): squared distances, the
assignment with its best-versus-second margin, per-cluster sums and counts, the k-means update with last_diff, and one
DP-means batch."""
import numpy as np


def sq_distances(x, ck):
    """[n, k] sums of squares, fp64, direct form."""
    x = np.asarray(x, np.float64).reshape(-1, np.shape(ck)[-1])
    c = np.asarray(ck, np.float64).reshape(-1, x.shape[1])
    out = np.empty((x.shape[0], c.shape[0]))
    for j0 in range(0, c.shape[0], 256):
        out[:, j0:j0 + 256] = ((x[:, None, :] - c[None, j0:j0 + 256, :]) ** 2).sum(axis=2)
    return out


def assign(x, ck):
    """(index, min_sq, margin): the lowest index of least distance, that distance, and the relative gap between the
    best and the second best (inf with one centroid)."""
    d = sq_distances(x, ck)
    index = d.argmin(axis=1)
    best = d[np.arange(d.shape[0]), index]
    if d.shape[1] == 1:
        return index, best, np.full(d.shape[0], np.inf)
    part = np.partition(d, 1, axis=1)
    margin = (part[:, 1] - part[:, 0]) / np.maximum(np.abs(part[:, 1]), 1e-30)
    return index, best, margin


def sums_counts(x, index, k):
    """fp64 per-cluster sums [k, d] and int64 counts [k]; rows with an index outside [0, k) are skipped."""
    x = np.asarray(x, np.float64)
    index = np.asarray(index).reshape(-1)
    keep = (index >= 0) & (index < k)
    sums = np.zeros((k, x.shape[1]))
    np.add.at(sums, index[keep], x[keep])
    return sums, np.bincount(index[keep], minlength=k).astype(np.int64)


def kmeans_update(ck, sums, counts, reg=1e-8):
    """(new centroids sums / (counts + reg), last_diff = max_j ||ck_j - new_j||)."""
    new = np.asarray(sums, np.float64) / (np.asarray(counts, np.float64)[:, None] + reg)
    return new, float(np.sqrt(((np.asarray(ck, np.float64).reshape(new.shape) - new) ** 2).sum(axis=1)).max())


def dpmeans_batch(x, mu, lam):
    """One fastDPMean batch: (index, mu after the batch, whether a centroid was added).  The distance is the norm; when
    its max exceeds lam the first row attaining it becomes a new centroid and takes its index."""
    index, best, _ = assign(x, mu)
    dist = np.sqrt(best)
    mu = np.asarray(mu, np.float64).reshape(-1, np.shape(x)[-1])
    if dist.max() > lam:
        i = int(dist.argmax())
        mu = np.concatenate([mu, np.asarray(x, np.float64)[i:i + 1]], axis=0)
        index = index.copy()
        index[i] = mu.shape[0] - 1
        return index, mu, True
    return index, mu, False
