"""The definition of CTC forced alignment (include/cpc2_hip.h, version 120) in numpy float64, vectorised over the states of a
frame: the same max-then-add order and the same tie rule as csrc/ctc_align.hip, so path, status, ties, score[0], first and last
are compared BY EQUALITY, tied cases included.

One sequence: logits x [T][k] (float32), targets y[0..L), blank = k - 1; states s in [0, 2 L + 1), sym(s) = blank for even s and
y[s // 2] for odd s.
  start  v[0][0] = x[0][blank]; v[0][1] = x[0][y0] when L >= 1; everything else -inf
  step   v[t][s] = max(v[t-1][s], v[t-1][s-1] when s >= 1, v[t-1][s-2] when s is odd, s >= 3 and y[s//2] != y[s//2 - 1])
                   + x[t][sym(s)], in float64, the max first, then one addition
  ties   among equal finite candidates s wins over s - 1 wins over s - 2; at the end 2 L wins over 2 L - 1 unless the latter is
         strictly larger; ties = 1 when a maximum on the returned path (the end included) had an equal finite competitor
  status 0 aligned; 1 no alignment: T < L + #{i: y[i] == y[i-1]}, or T = 0; 2 invalid: T outside [0, t_max], L outside
         [0, max_l], a label outside [0, k - 1).  With 1 or 2: path -1 everywhere, scores and lse NaN, first / last / conf
         -1 / -1 / NaN.

What is held to a bound instead: lse, score[1] and conf, whose values pass through exp and log.  With u = 2^-53, K classes,
n = ceil(K / 64) terms per lane of the device's wave and 6 merge steps, R_t = max_j x[t][j] - min_j x[t][j]:
  * the device's lse_t is an online max-shifted sum: a term reaches the total through its own exp, at most n + 6 rescalings
    (each an exp of a rounded difference and a product) and at most n + 6 additions.  No ulp figure is documented for the
    device's f64 exp and log; 2 ulp = 4 u each is ASSUMED.  A rounded difference d changes exp(d) by at most u |d| <= u R_t
    relative.  So the sum's relative error is at most rho_t = ((n + 6) (6 + R_t) + 4 + R_t) u, and
        B_lse[t] = rho_t + 4 u log K + u |lse_t|                               (log acc <= log K; the final m + log acc)
  * score[1] = score[0] - sum_t lse_t: any summation order of T terms errs by at most T u sum_t |lse_t|:
        B_score1 = sum_t B_lse[t] + T u sum_t |lse_t| + u |score[1]|
  * conf[i] = (sum over the token's m frames, in frame order, of x[t][y_i] - lse_t) / m, then one float32 rounding:
        B_conf[i] = (sum_t (B_lse[t] + u |term_t|) + m u sum_t |term_t|) / m + u |conf| + 2^-24 |conf|
This file's own float64 arithmetic (numpy's exp and log, a shorter chain of the same form) is covered by counting the float64
part of every bound TWICE.
"""
import numpy as np

U = 2.0 ** -53
ULP_EXP_LOG = 4 * U          # ASSUMED: 2 ulp for the device's f64 exp and log
NEG = -np.inf


def sym_table(y, blank):
    out = np.full(2 * len(y) + 1, blank, np.int64)
    out[1::2] = y
    return out


def needed_frames(y):
    y = np.asarray(y, np.int64)
    return len(y) + int((y[1:] == y[:-1]).sum())


def lse_bound(x, lse):
    """B_lse [T] for logits x [T][K] (already float64) and their log-sum-exp."""
    k = x.shape[1]
    n = -(-k // 64)
    r = x.max(axis=1) - x.min(axis=1)
    rho = ((n + 6) * (6 + r) + 4 + r) * U
    return 2 * (rho + ULP_EXP_LOG * np.log(k) + U * np.abs(lse))


def align(logits, t_len, y, t_max=None, max_l=None):
    """One sequence: logits [t_max][k] float32 (rows >= t_len are not looked at), y the targets (its length is L).  Returns a
    dict: status, ties, path [t_max] int32, score [2] float64, lse [t_max], first / last [max_l] int32, conf [max_l] float32, and
    the bounds b_lse [t_max], b_score1, b_conf [max_l]."""
    logits = np.asarray(logits)
    k = logits.shape[1]
    t_max = logits.shape[0] if t_max is None else t_max
    y = np.asarray(y, np.int64).reshape(-1)
    n_lab = len(y)
    max_l = n_lab if max_l is None else max_l
    blank = k - 1
    out = dict(status=0, ties=0, path=np.full(t_max, -1, np.int32), score=np.full(2, np.nan), lse=np.full(t_max, np.nan),
               first=np.full(max_l, -1, np.int32), last=np.full(max_l, -1, np.int32), conf=np.full(max_l, np.nan, np.float32),
               b_lse=np.zeros(t_max), b_score1=0.0, b_conf=np.zeros(max_l))
    if not 0 <= t_len <= t_max or not 0 <= n_lab <= max_l or ((y < 0) | (y >= blank)).any():
        out["status"] = 2
        return out
    if t_len == 0 or t_len < needed_frames(y):
        out["status"] = 1
        return out
    x = logits[:t_len].astype(np.float64)
    sym = sym_table(y, blank)
    n_states = len(sym)
    states = np.arange(n_states)
    allow2 = np.zeros(n_states, bool)
    allow2[3::2] = sym[3::2] != sym[1:-2:2]
    v = np.full(n_states, NEG)
    v[0] = x[0, blank]
    if n_lab:
        v[1] = x[0, y[0]]
    move = np.zeros((t_len, n_states), np.int8)
    tied = np.zeros((t_len, n_states), bool)
    with np.errstate(invalid="ignore"):
        for t in range(1, t_len):
            c1 = np.concatenate([[NEG], v[:-1]])
            c2 = np.where(allow2, np.concatenate([[NEG, NEG], v[:-2]])[:n_states], NEG)
            best = v
            gt1 = c1 > best
            tie = (c1 == best) & (best > NEG)
            best = np.where(gt1, c1, best)
            mv = np.where(gt1, 1, 0)
            gt2 = c2 > best
            tie = np.where(gt2, False, tie | ((c2 == best) & (best > NEG)))
            best = np.where(gt2, c2, best)
            mv = np.where(gt2, 2, mv)
            v = best + x[t, sym]                 # the max first, then one addition
            move[t], tied[t] = mv, tie
    s, met = n_states - 1, False
    if n_lab:
        if v[n_states - 2] > v[n_states - 1]:
            s = n_states - 2
        elif v[n_states - 2] == v[n_states - 1] and v[n_states - 1] > NEG:
            met = True
    assert v[s] > NEG
    score0 = v[s]
    path = out["path"]
    for t in range(t_len - 1, -1, -1):
        path[t] = s
        if t:
            met |= bool(tied[t, s])
            s -= int(move[t, s])
    assert s in (0, 1) and states[-1] == n_states - 1
    m = x.max(axis=1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    b_lse = lse_bound(x, lse)
    out["lse"][:t_len] = lse
    out["b_lse"][:t_len] = b_lse
    out["ties"] = int(met)
    out["score"][:] = [score0, score0 - lse.sum()]
    out["b_score1"] = float(b_lse.sum() + 2 * (t_len * U * np.abs(lse).sum() + U * abs(out["score"][1])))
    for i in range(n_lab):
        frames = np.nonzero(path[:t_len] == 2 * i + 1)[0]
        out["first"][i], out["last"][i] = frames[0], frames[-1]
        assert len(frames) == frames[-1] - frames[0] + 1
        terms = x[frames, y[i]] - lse[frames]
        acc = 0.0
        for term in terms:                       # in frame order
            acc += term
        conf = acc / len(frames)
        out["conf"][i] = np.float32(conf)
        out["b_conf"][i] = ((b_lse[frames] + 2 * U * np.abs(terms)).sum() + 2 * len(frames) * U * np.abs(terms).sum()) / len(frames) \
            + 2 * U * abs(conf) + 2.0 ** -24 * abs(conf)
    return out


def align_batch(logits, in_lengths, targets, tgt_lengths):
    """logits [b][t_max][k], targets [b][max_l] -> a list of align()'s dicts.  A target length outside [0, max_l] is status 2."""
    logits, targets = np.asarray(logits), np.asarray(targets).reshape(len(logits), -1)
    t_max, max_l = logits.shape[1], targets.shape[1]
    res = []
    for i in range(len(logits)):
        n_lab = int(tgt_lengths[i])
        if not 0 <= n_lab <= max_l:
            bad = align(logits[i], -1, [], t_max, max_l)
            assert bad["status"] == 2
            res.append(bad)
            continue
        res.append(align(logits[i], int(in_lengths[i]), targets[i, :n_lab], t_max, max_l))
    return res


def labels_of(path, y, blank):
    """The path mapped through sym; -1 where the path is -1."""
    path = np.asarray(path)
    table = sym_table(np.asarray(y, np.int64), blank)
    return np.where(path < 0, -1, table[np.clip(path, 0, len(table) - 1)])


def collapse(labels, blank):
    """Frame labels -> the label string: repeats merged, blanks removed."""
    out, prev = [], None
    for a in labels:
        if a != prev and a != blank:
            out.append(int(a))
        prev = a
    return out
