"""numpy float64 oracles of cpc2_amd.cca: the second moments of two data matrices, and sklearn's CCA algorithm (NIPALS, PLS
mode B, canonical deflation, scale=True) run on the DATA MATRICES themselves -- SVD pseudo-inverses of the [n, d] matrices and
explicit deflation of Xk, Yk -- a formulation independent of the library's covariance-space one."""
import warnings

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def moments(X, Y=None):
    """(n, sx, sy, Sxx, Sxy, Syy) in float64 (Y None: sy, Sxy, Syy empty)."""
    X = np.asarray(X, np.float64)
    Y = np.zeros((X.shape[0], 0)) if Y is None else np.asarray(Y, np.float64)
    return X.shape[0], X.sum(0), Y.sum(0), X.T @ X, X.T @ Y, Y.T @ Y


def moments_bound(X, Y=None):
    """First-order bound of an f64 sum of n exact products, doubled because the oracle rounds too:
    (bound of sums [D], bound of gram [D, D]) for Z = [X, Y]."""
    Z = np.abs(np.asarray(X, np.float64))
    if Y is not None:
        Z = np.concatenate([Z, np.abs(np.asarray(Y, np.float64))], axis=1)
    u = 2.0 * Z.shape[0] * 2.0 ** -53
    return u * Z.sum(0), u * (Z.T @ Z)


def _pinv_data(a):
    u, s, vh = np.linalg.svd(a, full_matrices=False)
    rank = int(np.sum(s > s.max() * 1e6 * EPS))
    return (vh[:rank].T / s[:rank]) @ u[:, :rank].T


def cca_fit(X, Y, n_components, max_iter=500, tol=1e-06):
    """dict of sklearn's fitted attributes (and n_iter_)."""
    X, Y = np.array(X, np.float64), np.array(Y, np.float64)
    n, p = X.shape
    q = Y.shape[1]
    x_mean, y_mean = X.mean(0), Y.mean(0)
    X -= x_mean
    Y -= y_mean
    x_std, y_std = X.std(0, ddof=1), Y.std(0, ddof=1)
    x_std[x_std == 0.0] = 1.0
    y_std[y_std == 0.0] = 1.0
    X /= x_std
    Y /= y_std
    W, V = np.zeros((p, n_components)), np.zeros((q, n_components))
    P, Q = np.zeros((p, n_components)), np.zeros((q, n_components))
    n_iter = []
    for k in range(n_components):
        Y[:, np.all(np.abs(Y) < 10 * EPS, axis=0)] = 0.0
        start = [j for j in range(q) if np.any(np.abs(Y[:, j]) > EPS)]
        if not start:
            warnings.warn(f"y residual is constant at iteration {k}")
            break
        y_score = Y[:, start[0]]
        Xp, Yp = _pinv_data(X), _pinv_data(Y)
        w_old = 100.0
        for i in range(max_iter):
            w = Xp @ y_score
            w /= np.sqrt(w @ w) + EPS
            x_score = X @ w
            v = Yp @ x_score
            v /= np.sqrt(v @ v) + EPS
            y_score = Y @ v / (v @ v + EPS)
            if (w - w_old) @ (w - w_old) < tol or q == 1:
                break
            w_old = w
        n_iter.append(i + 1)
        sign = np.sign(w[np.argmax(np.abs(w))])
        w, v = w * sign, v * sign
        t, u = X @ w, Y @ v
        pk, qk = t @ X / (t @ t), u @ Y / (u @ u)
        X -= np.outer(t, pk)
        Y -= np.outer(u, qk)
        W[:, k], V[:, k], P[:, k], Q[:, k] = w, v, pk, qk
    x_rot = W @ np.linalg.pinv(P.T @ W, rcond=n_components * EPS)
    y_rot = V @ np.linalg.pinv(Q.T @ V, rcond=n_components * EPS)
    coef = ((x_rot @ Q.T) * y_std).T / x_std
    return dict(x_weights_=W, y_weights_=V, x_loadings_=P, y_loadings_=Q, x_rotations_=x_rot, y_rotations_=y_rot, coef_=coef,
                intercept_=y_mean, n_iter_=np.asarray(n_iter, np.int64), _x_mean=x_mean, _y_mean=y_mean, _x_std=x_std,
                _y_std=y_std)


ATTRIBUTES = ("x_weights_", "y_weights_", "x_loadings_", "y_loadings_", "x_rotations_", "y_rotations_", "coef_", "intercept_",
              "_x_mean", "_y_mean", "_x_std", "_y_std")


def deviation(got, golden, tag):
    """Largest |got - golden| over the attributes, each relative to the golden attribute's largest magnitude.  `got` is a
    mapping or an object with the attributes; `golden` the loaded g28 file."""
    worst = 0.0
    for name in ATTRIBUTES:
        ref = golden[f"{tag}_{name}"]
        val = got[name] if isinstance(got, dict) else getattr(got, name)
        assert np.shape(val) == ref.shape, (tag, name, np.shape(val), ref.shape)
        worst = max(worst, float(np.abs(np.asarray(val) - ref).max() / np.abs(ref).max()))
    return worst
