"""The definition cpc_unit_counts / cpc_unit_boundaries (csrc/unit_scores.hip), cpc2_amd.unit_scores and the unit_quality tool are
held to, in numpy and plain Python, written without looking at the module.  The reference has no such tool: this file is the
specification (phone purity, cluster purity and PNMI as in Hsu et al. 2021, HuBERT, section IV-A; the bitrate of Dunbar et al. 2019,
ZeroSpeech 2019: n H(symbols) / D bits per second).

TABLES (tables): an utterance compares `length` frames: unit z[f] and label y[f] (label 0 everywhere without labels).  A frame with
z outside [0, n_units) or y outside [0, n_phones) adds 1 to `invalid` and to nothing else.  Every other frame adds 1 to joint[z][y],
1 to unit_runs[z] when f == 0 or z[f] != z[f-1], 1 to phone_runs[y] when f == 0 or y[f] != y[f-1] (the frame before is compared as
it stands, valid or not).  Explicit loops and np.add.at; all integers: the device must EQUAL them.
BOUNDARIES (boundaries): hypotheses = frames f in [1, length - 1] with z[f] != z[f-1], references the same for y; the five counts
(n_ref, n_hyp, hits, hyp_near, ref_near) with `match` and `counts` of segmentation_oracle.py.

SCORES (scores): N = joint.sum(), p(y, z) = Fraction(joint[z][y], N); every probability is an exact Fraction, every logarithm
math.log2 of the float nearest to an exact Fraction, every sum math.fsum.

THE BOUND (score_bounds).  u = 2^-53.  A term of an entropy or of MI is t = p * log2(q) with p and q exact rationals (q = p for an
entropy, q = p(y, z) / (p(y) p(z)) for MI).  An evaluation in float64 performs, per term:
    1. p rounded to a float: relative u, moves t by u |t|
    2. q rounded to a float: relative u in the argument of log2, moves log2(q) by at most u / ln 2 < 1.5 u, and t by 1.5 u p
    3. log2 itself, ASSUMED within 1 ulp = 2 u relative of the true logarithm of its argument (the C library's claim): 2 u |t|
    4. the product: u |t|
so one evaluation of a term is within u (4 |t| + 1.5 p) of the exact term, to first order (u^2 ignored: 1e-32).  math.fsum adds the
computed terms exactly and rounds once: u |S|.  A sum S of such terms is therefore within
    e(S) = u (4 sum |t| + 1.5 sum p + |S|)
of its exact value, and two evaluations (this file's and the module's) are within 2 e(S) of each other WHATEVER the order of their
operations, as long as each performs those four roundings per term and one correctly rounded sum.  That is what is asserted: no
figure was fitted.  For an entropy sum p = 1 and sum |t| = H: e(H) = u (5 H + 1.5).  When q is exactly 1 (an outer-product joint)
log2 gives exactly 0 and the term is exactly 0.
Derived scores, by first-order propagation plus their own roundings (each u relative, counted below):
    purity          sum of max counts / N: one rounding per term and one of fsum: e = 2 u S
    pnmi = MI / H   (e(MI) + pnmi e(H)) / H + u pnmi
    perplexity      2 ** H: ln 2 * 2^H * e(H) + 2 u 2^H (pow ASSUMED within 1 ulp)
    bitrate         N H / (N feature_size): three roundings (two products, one division) on top of e(H): value (e(H) / H + 3 u)
    mean run        N / R: ONE correctly rounded division of two integers: both evaluations give the same float (bound 0)
    boundary scores the Python-float formulas of segmentation_oracle.boundary_scores on equal integers: the same IEEE operations in
                    the same order (bound 0)
Every bound is doubled for the distance between two evaluations.
"""
import math
from fractions import Fraction

import numpy as np

import segmentation_oracle as SO

U53 = 2.0 ** -53


def tables(units, labels, n_units, n_phones):
    """units, labels: one integer sequence per utterance, already cut to the compared length (labels None: label 0 everywhere)
    -> (joint int64 [n_units, n_phones], unit_runs [n_units], phone_runs [n_phones], invalid int)."""
    joint = np.zeros((n_units, n_phones), np.int64)
    unit_runs = np.zeros(n_units, np.int64)
    phone_runs = np.zeros(n_phones, np.int64)
    invalid = 0
    for i, z in enumerate(units):
        z = np.asarray(z, dtype=np.int64)
        y = np.zeros(len(z), np.int64) if labels is None else np.asarray(labels[i], dtype=np.int64)
        assert len(y) == len(z)
        ok = (z >= 0) & (z < n_units) & (y >= 0) & (y < n_phones)
        invalid += int((~ok).sum())
        np.add.at(joint, (z[ok], y[ok]), 1)
        for f in range(len(z)):
            if not ok[f]:
                continue
            if f == 0 or z[f] != z[f - 1]:
                unit_runs[z[f]] += 1
            if f == 0 or y[f] != y[f - 1]:
                phone_runs[y[f]] += 1
    return joint, unit_runs, phone_runs, invalid


def change_points(seq):
    return [f for f in range(1, len(seq)) if seq[f] != seq[f - 1]]


def boundaries(units, labels, tol):
    """(n_ref, n_hyp, hits, hyp_near, ref_near) of one utterance (labels None: no reference)."""
    hyp = change_points(list(units))
    ref = change_points(list(labels)) if labels is not None else []
    n_hyp, hits, hyp_near, ref_near = SO.counts(ref, hyp, tol)
    return [len(ref), n_hyp, hits, hyp_near, ref_near]


def _plogq(pairs):
    """sum p log2 q over (p, q) exact Fractions, p > 0 -> (sum, e(S) of the module docstring)."""
    terms = [float(p) * math.log2(q) for p, q in pairs]
    s = math.fsum(terms)
    err = U53 * (4 * math.fsum(abs(t) for t in terms) + 1.5 * math.fsum(float(p) for p, _q in pairs) + abs(s))
    return s, err


def _entropy(counts):
    total = int(sum(int(c) for c in counts))
    if total == 0:
        return 0.0, 0.0
    s, err = _plogq([(Fraction(int(c), total),) * 2 for c in counts if c])
    return -s, err


def scores(joint, unit_runs, phone_runs, boundary_rows=None, tol=2, feature_size=0.01, has_labels=True):
    """(scores dict, bounds dict): the bound of every float entry as the distance allowed between two evaluations."""
    joint = np.asarray(joint, dtype=np.int64)
    n = int(joint.sum())
    nz = [int(v) for v in joint.sum(axis=1)]
    ny = [int(v) for v in joint.sum(axis=0)]
    h_unit, e_hu = _entropy(nz)
    r = int(np.sum(unit_runs))
    h_runs, e_hr = _entropy([int(v) for v in unit_runs])
    out = {"n_frames": n, "n_units": joint.shape[0], "used_units": sum(1 for v in nz if v), "H_unit": h_unit,
           "perplexity": 2.0 ** h_unit, "bitrate_frames": n * h_unit / (n * feature_size),
           "bitrate_runs": r * h_runs / (n * feature_size), "mean_unit_run": float(Fraction(n, r)), "n_unit_runs": r}
    bound = {"H_unit": 2 * e_hu, "perplexity": 2 * (math.log(2) * out["perplexity"] * e_hu + 2 * U53 * out["perplexity"]),
             "bitrate_frames": 2 * (n * e_hu / (n * feature_size) + 3 * U53 * out["bitrate_frames"]),
             "bitrate_runs": 2 * (r * e_hr / (n * feature_size) + 3 * U53 * out["bitrate_runs"]), "mean_unit_run": 0.0}
    if not has_labels:
        return out, bound
    h_phone, e_hp = _entropy(ny)
    pairs = []
    for z in range(joint.shape[0]):
        for y in range(joint.shape[1]):
            c = int(joint[z, y])
            if c:
                p = Fraction(c, n)
                pairs.append((p, p / (Fraction(ny[y], n) * Fraction(nz[z], n))))
    mi, e_mi = _plogq(pairs)
    phone_purity = math.fsum(float(Fraction(int(joint[z].max()), n)) for z in range(joint.shape[0]))
    cluster_purity = math.fsum(float(Fraction(int(joint[:, y].max()), n)) for y in range(joint.shape[1]))
    pnmi = mi / h_phone if h_phone > 0 else float("nan")
    n_phone_runs = int(np.sum(phone_runs))
    out.update({"n_phones": joint.shape[1], "phone_purity": phone_purity, "cluster_purity": cluster_purity, "H_phone": h_phone,
                "MI": mi, "pnmi": pnmi, "mean_phone_run": float(Fraction(n, n_phone_runs)), "n_phone_runs": n_phone_runs})
    bound.update({"phone_purity": 4 * U53 * phone_purity, "cluster_purity": 4 * U53 * cluster_purity, "H_phone": 2 * e_hp,
                  "MI": 2 * e_mi, "mean_phone_run": 0.0,
                  "pnmi": 2 * ((e_mi + abs(pnmi) * e_hp) / h_phone + U53 * abs(pnmi)) if h_phone > 0 else 0.0})
    if boundary_rows is not None:
        n_ref, n_hyp, hits, hyp_near, ref_near = (int(v) for v in np.asarray(boundary_rows, dtype=np.int64).reshape(-1, 5).sum(axis=0))
        out["boundaries"] = {"tolerance": tol, "n_ref": n_ref, "n_hyp": n_hyp, "hits": hits, "hyp_near": hyp_near,
                             "ref_near": ref_near, "strict": SO.boundary_scores(n_ref, n_hyp, hits),
                             "lenient": SO.boundary_scores(n_ref, n_hyp, hyp_near, ref_hits=ref_near)}
    return out, bound


def unit_to_phone(joint):
    """[(unit, majority phone (lowest index on ties), its count, the unit's frames, purity)] over the used units."""
    out = []
    for z, row in enumerate(np.asarray(joint, dtype=np.int64)):
        tot = int(row.sum())
        if tot == 0:
            continue
        best = 0
        for y in range(len(row)):
            if row[y] > row[best]:
                best = y
        out.append((z, best, int(row[best]), tot, float(Fraction(int(row[best]), tot))))
    return out


def assert_scores_close(got, want, bound):
    """Every entry of `got` against the oracle's: integers and the bound-0 floats by ==, floats within their bound, NaN with NaN."""
    assert set(got) == set(want), set(got) ^ set(want)
    for key, w in want.items():
        g = got[key]
        if isinstance(w, dict):
            assert_scores_close(g, w, {})
        elif isinstance(w, float) and math.isnan(w):
            assert math.isnan(g), key
        elif isinstance(w, float):
            assert abs(g - w) <= bound.get(key, 0.0), (key, g, w, bound.get(key, 0.0))
        else:
            assert g == w, (key, g, w)
