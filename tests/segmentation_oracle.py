"""The definition cpc_seg_dissimilarity / cpc_seg_boundaries (csrc/segment.hip) and cpc2_amd.segmentation are held to, in float64
numpy and plain Python.  The reference has no segmentation tool: this file is the specification (the recipe of Kreuk et al. 2020,
"Self-supervised contrastive learning for unsupervised phoneme segmentation", with the R-value of Rasanen et al. 2009).  The peak
and prominence rules are those of scipy.signal.find_peaks / peak_prominences with wlen=None; scipy is NOT imported here
(test_segmentation_cpu.py compares the two where scipy is installed).

One utterance: frames x[0..L) float32 of D columns, labels l[0..L') (optional), thresholds p[0..K), tolerance tol in frames.

1. d[t] = 1 - dot(x_t, x_t+1) / sqrt(|x_t|^2 |x_t+1|^2) for t < L - 1; d[t] = 1 when the product of the squared norms is 0.  The
   three sums are float64 sums of the float32 inputs' products (each product of two float32 values is exact in float64).  An
   utterance with a non-finite feature has status 2 and no boundaries.
2. Peaks of d (n = L - 1 entries): index i in [1, n - 2] starts a peak when d[i-1] < d[i]; scan ahead over the entries equal to
   d[i]; the run is a peak if the entry behind it exists and is smaller, at position (left + right) // 2.
3. Prominence of a peak at q: walk left from q while d[i] <= d[q], keeping the minimum; the same to the right;
   prom = d[q] - max(left minimum, right minimum).
4. A peak is kept at threshold p when prom >= p * (max d - min d); a kept peak at q is a boundary at frame q + 1.
5. Reference boundaries: frames f in [1, n_l - 1] with l[f] != l[f-1], n_l = min(L, L'); hypotheses at frames >= n_l are dropped.
6. Counts per threshold: n_hyp, hits (two-pointer one-to-one matching), hyp_near, ref_near.
7. Scores from integer totals: boundary_scores.

THE BOUND OF STEP 1 (dissimilarity_bound).  u = 2^-53.  A float64 sum of D exact products, in ANY order, differs from the true sum
by at most (D - 1) u sum |terms| to first order.  With c = dot / sqrt(na nb) and |c| <= 1, sum |x_i y_i| <= sqrt(na nb):
    the dot product's sum               moves c by at most (D - 1) u
    the two norms' sums                 are each relative (D - 1) u, their product 2 (D - 1) u, its square root (D - 1) u
    the product na nb                   one rounding u, halved by the square root: u / 2
    the square root and the division    ASSUMED within 1 ulp = 2 u relative each on the device (correctly rounded here: u)
    the subtraction 1 - c               one rounding of d, |d| <= 2: 2 u
One evaluation is therefore within (2 (D - 1) + 1 / 2 + 2 + 2 + 2) u = (2 D + 4.5) u of the true value, and two evaluations (this
file's and the device's) within (4 D + 9) u of each other.  Second-order terms (D^2 u^2) are ignored: at D = 260 they are 1e-27.
"""
import math

import numpy as np

U53 = 2.0 ** -53
FRAME_SECONDS = 160 / 16000


def dissimilarity_bound(dim):
    """|d_device - d_oracle| <= (4 D + 9) 2^-53 (module docstring)."""
    return (4 * dim + 9) * U53


def dissimilarity(x):
    """(d float64 [max(L - 1, 0)], status): step 1.  status 2: a non-finite feature (the pairs of such a row are NaN)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    n = max(x.shape[0] - 1, 0)
    status = 0 if np.isfinite(x).all() else 2
    if n == 0:
        return np.zeros(0, np.float64), status
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        norm = (x64 * x64).sum(axis=1)
        dot = (x64[:-1] * x64[1:]).sum(axis=1)
        prod = norm[:-1] * norm[1:]
        d = np.ones(n, np.float64)
        live = prod != 0.0
        d[live] = 1.0 - dot[live] / np.sqrt(prod[live])
    d[~np.isfinite(norm[:-1]) | ~np.isfinite(norm[1:])] = np.nan
    return d, status


def local_maxima(d):
    """Positions of the peaks of d (step 2), increasing."""
    n = len(d)
    peaks = []
    i = 1
    while i < n - 1:
        if d[i - 1] < d[i]:
            ahead = i + 1
            while ahead < n and d[ahead] == d[i]:
                ahead += 1
            if ahead < n and d[ahead] < d[i]:
                peaks.append((i + ahead - 1) // 2)
            i = ahead
        else:
            i += 1
    return peaks


def prominence(d, q):
    """Step 3: one subtraction of two entries of d."""
    left = right = d[q]
    i = q
    while i >= 0 and d[i] <= d[q]:
        left = min(left, d[i])
        i -= 1
    i = q
    while i < len(d) and d[i] <= d[q]:
        right = min(right, d[i])
        i += 1
    return d[q] - max(left, right)


def peaks_and_prominences(d):
    """(peaks int list, prominences float64 list, range): range = max d - min d, 0.0 for an empty d."""
    d = np.asarray(d, dtype=np.float64)
    peaks = local_maxima(d)
    proms = [np.float64(prominence(d, q)) for q in peaks]
    rng = np.float64(d.max() - d.min()) if len(d) else np.float64(0.0)
    return peaks, proms, rng


def select(peaks, proms, rng, p, limit=None):
    """Step 4: the boundary frames kept at threshold p (one product), those at frames >= limit dropped."""
    cut = np.float64(p) * np.float64(rng)
    return [q + 1 for q, pr in zip(peaks, proms) if pr >= cut and (limit is None or q + 1 < limit)]


def reference_boundaries(labels, n):
    """Step 5: frames f in [1, n - 1] with labels[f] != labels[f - 1]."""
    return [f for f in range(1, n) if labels[f] != labels[f - 1]]


def match(ref, hyp, tol):
    """Step 6's one-to-one matching by two pointers over the sorted lists."""
    i = j = hits = 0
    while i < len(ref) and j < len(hyp):
        if abs(hyp[j] - ref[i]) <= tol:
            hits, i, j = hits + 1, i + 1, j + 1
        elif hyp[j] < ref[i]:
            j += 1
        else:
            i += 1
    return hits


def counts(ref, hyp, tol):
    """(n_hyp, hits, hyp_near, ref_near): hyp_near = hypotheses with some reference within tol, ref_near = references with some
    hypothesis within tol (every pair is looked at)."""
    near = np.abs(np.subtract.outer(np.asarray(hyp, dtype=np.int64), np.asarray(ref, dtype=np.int64))) <= tol
    return len(hyp), match(ref, hyp, tol), int(near.any(axis=1).sum()), int(near.any(axis=0).sum())


def boundary_scores(n_ref, n_hyp, hits, ref_hits=None):
    """Step 7 from integer totals, in Python floats.  The lenient scores: hits = hyp_near, ref_hits = ref_near."""
    precision = hits / n_hyp if n_hyp else 0.0
    recall = (hits if ref_hits is None else ref_hits) / n_ref if n_ref else 0.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    over = n_hyp / n_ref - 1 if n_ref else float("nan")
    r1 = math.sqrt((1 - recall) ** 2 + over ** 2)
    r2 = (recall - 1 - over) / math.sqrt(2)
    return {"precision": precision, "recall": recall, "f1": f1, "os": over, "rval": 1 - (abs(r1) + abs(r2)) / 2}


def segment(d, thresholds, ref=None, tol=2, limit=None):
    """Steps 2-6 on one utterance's d -> dict(status, peaks, proms, range, counts [K][4]).  Non-finite d: status 2, nothing else."""
    d = np.asarray(d, dtype=np.float64)
    k = len(thresholds)
    if not np.isfinite(d).all():
        return {"status": 2, "peaks": [], "proms": [], "range": np.float64(np.nan), "counts": [[0, 0, 0, 0]] * k}
    peaks, proms, rng = peaks_and_prominences(d)
    out = []
    for p in thresholds:
        hyp = select(peaks, proms, rng, p, limit if limit is not None else len(d) + 1)
        out.append(list(counts(ref, hyp, tol)) if ref is not None else [len(hyp), 0, 0, 0])
    return {"status": 0, "peaks": peaks, "proms": proms, "range": rng, "counts": out}


def margin(d, thresholds):
    """How far the case is from a decision that arithmetic error could move: the smaller of the smallest gap between two DISTINCT
    values of d and the smallest |prom - p * range| over peaks and thresholds (inf where there is neither)."""
    d = np.asarray(d, dtype=np.float64)
    values = np.unique(d)
    gap = float(np.diff(values).min()) if len(values) > 1 else float("inf")
    peaks, proms, rng = peaks_and_prominences(d)
    near = min((abs(float(pr) - float(p) * float(rng)) for pr in proms for p in thresholds), default=float("inf"))
    return min(gap, near)


def boundary_times(frames):
    return [f * FRAME_SECONDS for f in frames]
