"""fp64 numpy oracle of the probe heads (cpc2_amd/csrc/probe.hip), independent of torch: softmax cross-entropy with its
gradients, CTC (blank = K - 1, zero_infinity, reduction 'mean') as a log-space alpha-beta, and the label collapse."""
import numpy as np


def xent(x, w, b, labels):
    """loss (mean nll), accuracy (first index wins ties), dW, db, dX of logits = x W^T + b -- all float64."""
    x, w, b = (np.asarray(a, np.float64) for a in (x, w, b))
    labels = np.asarray(labels, np.int64)
    n = x.shape[0]
    z = x @ w.T + b
    m = z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
    nll = lse - z[np.arange(n), labels]
    pred = z.argmax(axis=1)                          # (numpy: the first maximum)
    p = np.exp(z - lse[:, None])
    p[np.arange(n), labels] -= 1.0
    dz = p / n
    return dict(loss=nll.mean(), nll=nll, acc=float((pred == labels).mean()), pred=pred, logits=z, dz=dz,
                dW=dz.T @ x, db=dz.sum(axis=0), dX=dz @ w)


def _lae(a, b):
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        return np.where(m == -np.inf, -np.inf, m + np.log1p(np.exp(np.minimum(a, b) - m)))


def ctc_one(logits, target):
    """(nll, dlogits) of one sequence, logits [T, K] (blank = K - 1), unscaled: nll = -log p, grad = softmax - occupancy;
    (inf, zeros) when no alignment exists."""
    z = np.asarray(logits, np.float64)
    T, K = z.shape
    blank = K - 1
    m = z.max(axis=1, keepdims=True)
    lp = z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))
    ext = np.full(2 * len(target) + 1, blank, np.int64)
    ext[1::2] = target
    S = len(ext)
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    alpha = np.full((T, S), -np.inf)
    alpha[0, 0] = lp[0, blank]
    if S > 1:
        alpha[0, 1] = lp[0, ext[1]]
    for t in range(1, T):
        a = alpha[t - 1].copy()
        a[1:] = _lae(a[1:], alpha[t - 1, :-1])
        a[2:] = np.where(skip[2:], _lae(a[2:], alpha[t - 1, :-2]), a[2:])
        alpha[t] = a + lp[t, ext]
    beta = np.full((T, S), -np.inf)
    beta[T - 1, S - 1] = lp[T - 1, ext[S - 1]]
    if S > 1:
        beta[T - 1, S - 2] = lp[T - 1, ext[S - 2]]
    for t in range(T - 2, -1, -1):
        bt = beta[t + 1].copy()
        bt[:-1] = _lae(bt[:-1], beta[t + 1, 1:])
        bt[:-2] = np.where(skip[2:], _lae(bt[:-2], beta[t + 1, 2:]), bt[:-2])
        beta[t] = bt + lp[t, ext]
    logp = _lae(alpha[T - 1, S - 1], alpha[T - 1, S - 2] if S > 1 else -np.inf)
    if logp == -np.inf:
        return np.inf, np.zeros((T, K))
    ab = alpha + beta
    occ = np.zeros((T, K))
    for k in range(K):
        sel = ext == k
        if sel.any():
            mm = ab[:, sel].max(axis=1)
            ok = mm > -np.inf
            s = np.zeros(T)
            s[ok] = np.exp(mm[ok] + np.log(np.exp(ab[ok][:, sel] - mm[ok, None]).sum(axis=1)) - logp - lp[ok, k])
            occ[:, k] = s
    return -logp, np.exp(lp) - occ


def ctc(logits, targets, lengths):
    """nn.CTCLoss(blank=K-1, reduction='mean', zero_infinity=True) of log_softmax(logits [B, T, K]): (loss, nll [B] with
    infinities zeroed, dlogits [B, T, K])."""
    B = logits.shape[0]
    nll = np.zeros(B)
    grad = np.zeros(logits.shape)
    loss = 0.0
    for i in range(B):
        L = int(lengths[i])
        v, g = ctc_one(logits[i], np.asarray(targets[i][:L], np.int64))
        if np.isinf(v):
            v, g = 0.0, np.zeros_like(g)
        nll[i] = v
        grad[i] = g / (B * max(L, 1))
        loss += v / max(L, 1)
    return loss / B, nll, grad


def collapse(labels):
    """collapseLabelChain: (padded [N, maxS] int64, sizes [N])."""
    labels = np.asarray(labels, np.int64)
    rows = [r[np.concatenate([[True], r[1:] != r[:-1]])] for r in labels]
    sizes = np.array([len(r) for r in rows], np.int64)
    out = np.zeros((len(rows), sizes.max() if len(rows) else 0), np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, sizes
