"""The numpy float64 statement of duration-penalized unit segmentation (include/cpc2_hip.h, version 129),
a direct transcription of the definition:

    V[0][k] = (double) c[0][k]
    m[t]    = min_k V[t][k]          a[t] = the LOWEST k with V[t][k] == m[t]
    sw      = m[t-1] + lambda                                  (one f64 add)
    stay[t][k] = (V[t-1][k] <= sw)                             (a tie stays)
    V[t][k] = (double) c[t][k] + (stay[t][k] ? V[t-1][k] : sw) (one f64 add)
    u[T-1] = a[T-1];  u[t-1] = stay[t][u[t]] ? u[t] : a[t-1]

Every line is one IEEE operation on float64 arrays; nothing is fused and nothing is reordered, so the device must EQUAL it.
"""
import itertools

import numpy as np

DONE, EMPTY, NONFINITE, OUTSIDE = 0, 1, 2, 3


def segment(cost, lam):
    """One utterance: cost [T, K] float32, lam a float64 >= 0 -> (units int32 [T], energy float64, n_segments, status)."""
    cost = np.asarray(cost, dtype=np.float32)
    T = cost.shape[0]
    if T <= 0:
        return np.zeros(0, np.int32), 0.0, 0, EMPTY
    if not np.isfinite(cost).all():
        return np.full(T, -1, np.int32), float("nan"), 0, NONFINITE
    lam = np.float64(lam)
    c = cost.astype(np.float64)
    V = c[0].copy()
    a = np.zeros(T, np.int64)
    stay = np.ones(cost.shape, dtype=bool)
    a[0] = np.argmin(V)                                  # (the first minimum: the lowest index; -0.0 == +0.0)
    m = V[a[0]]
    for t in range(1, T):
        sw = m + lam
        stay[t] = V <= sw
        V = c[t] + np.where(stay[t], V, sw)
        a[t] = np.argmin(V)
        m = V[a[t]]
    u = np.zeros(T, np.int32)
    u[T - 1] = a[T - 1]
    for t in range(T - 1, 0, -1):
        u[t - 1] = u[t] if stay[t][u[t]] else a[t - 1]
    return u, float(m), 1 + int((u[1:] != u[:-1]).sum()), DONE


def segment_pack(cost, offsets, lengths, penalties, k=None):
    """The entry point's outputs for a pack: cost [n_rows, ld] float32 -> (units [n_pen, n_rows] int32 with -2 where nothing is
    written, energy [n_pen, n_utt], n_segments, status)."""
    cost = np.asarray(cost, dtype=np.float32)
    n_rows = cost.shape[0]
    k = cost.shape[1] if k is None else k
    n_pen, n_utt = len(penalties), len(lengths)
    units = np.full((n_pen, n_rows), -2, np.int32)
    energy = np.zeros((n_pen, n_utt), np.float64)
    n_seg = np.zeros((n_pen, n_utt), np.int32)
    status = np.zeros((n_pen, n_utt), np.int32)
    for i, (off, T) in enumerate(zip(offsets, lengths)):
        off, T = int(off), int(T)
        for p, lam in enumerate(penalties):
            if T <= 0:
                energy[p, i], n_seg[p, i], status[p, i] = 0.0, 0, EMPTY
            elif off < 0 or off + T > n_rows or T > 1 << 24:
                energy[p, i], n_seg[p, i], status[p, i] = np.nan, 0, OUTSIDE
            else:
                u, e, s, st = segment(cost[off:off + T, :k], lam)
                units[p, off:off + T] = u
                energy[p, i], n_seg[p, i], status[p, i] = e, s, st
    return units, energy, n_seg, status


def brute_force(cost, lam):
    """min over all K^T labelings of sum_t c[t][u_t] + lam (S - 1), in exact integers (the caller passes integers)."""
    cost = np.asarray(cost)
    T, K = cost.shape
    best = None
    for lab in itertools.product(range(K), repeat=T):
        s = 1 + sum(1 for t in range(1, T) if lab[t] != lab[t - 1])
        e = sum(int(cost[t, lab[t]]) for t in range(T)) + int(lam) * (s - 1)
        best = e if best is None or e < best else best
    return best


def labeling_energy(cost, units, lam):
    """sum_t c[t][u_t] + lam (S - 1) of one labeling, in exact integers."""
    cost = np.asarray(cost)
    s = 1 + sum(1 for t in range(1, len(units)) if units[t] != units[t - 1])
    return sum(int(cost[t, units[t]]) for t in range(len(units))) + int(lam) * (s - 1)
