"""Canonical correlation analysis between two feature streams, from their second moments alone.

The reference fits sklearn.cross_decomposition.CCA on every frame of both models held on the host.  The same algorithm (NIPALS,
PLS mode B, canonical deflation, scale=True) needs only the count, the column sums and X^T X, X^T Y, Y^T Y of the two streams:

    Moments            accumulates them on the device, batch by batch, in f64 (cpc_moments_accumulate: exact products of the
                       f32 inputs summed on the f64 matrix instruction, deterministic, O(D^2) memory);
    cca_from_moments   runs the iterations on d x d matrices in numpy float64 on the host;
    CCAModel           holds the fitted attributes under sklearn's names, transforms device tensors through cpc_gemm_nt and
                       is saved as an .npz (no pickle);
    to_sklearn         rebuilds a sklearn CCA object from it, where sklearn is installed, for the reference's .pkl.

No scipy or sklearn import outside to_sklearn.
"""
import warnings

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, require_gpu, scratch, stream_ptr

MAX_DIM = 512            # per stream (cpc_moments_accumulate)
_EPS = float(np.finfo(np.float64).eps)


# --------------------------------------------------------------------------- the moments, on the device
def _rows(t, d, name):
    """(tensor kept alive, row stride in elements, rows) of a float32 [n, d] / [b, s, d] tensor; a row stride is passed on as ld,
    anything else is made contiguous."""
    if t.dtype != torch.float32:
        raise TypeError(f"cpc2_amd kernels are fp32 only (got {t.dtype} for {name})")
    if t.dim() not in (2, 3) or t.shape[-1] != d:
        raise ValueError(f"{name}: expected [n, {d}] or [b, s, {d}], got {tuple(t.shape)}")
    if t.dim() == 3:
        b, s, _ = t.shape
        if t.stride(2) == 1 and t.stride(1) >= d and t.stride(0) == s * t.stride(1):
            return t, t.stride(1), b * s
        t = t.contiguous()
        return t, d, b * s
    if t.stride(1) == 1 and (t.stride(0) >= d or t.shape[0] <= 1):
        return t, max(t.stride(0), d), t.shape[0]
    t = t.contiguous()
    return t, d, t.shape[0]


class Moments:
    """Running count, column sums and Gram matrix of the rows z = [x row, y row] (dy = 0: of x alone)."""

    def __init__(self, dx, dy=0, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"cpc2_amd runs only on a GPU (HIP) device: got '{device}'. There is no CPU fallback.")
        if not (1 <= dx <= MAX_DIM and 0 <= dy <= MAX_DIM):
            raise ValueError(f"Moments: widths outside the supported limits (dx={dx} dy={dy}; need 1 <= dx <= {MAX_DIM}, "
                             f"0 <= dy <= {MAX_DIM})")
        self.dx, self.dy = int(dx), int(dy)
        self.device = device
        self.count = 0
        d = self.dx + self.dy
        self.sums = torch.zeros(d, dtype=torch.float64, device=device)
        self.gram = torch.zeros(d, d, dtype=torch.float64, device=device)

    def update(self, x, y=None):
        require_gpu(x, y)
        if (y is None) != (self.dy == 0):
            raise ValueError("Moments.update: y is given exactly when dy > 0")
        x, ldx, n = _rows(x, self.dx, "x")
        ldy = 0
        if y is not None:
            y, ldy, ny = _rows(y, self.dy, "y")
            if ny != n:
                raise ValueError(f"Moments.update: x has {n} rows and y has {ny}")
        if n == 0:
            return self
        lib = _lib.load()
        nb = lib.cpc_moments_scratch_bytes(n, self.dx, self.dy)
        check(lib.cpc_moments_accumulate(ptr(x), ldx, self.dx, ptr(y), ldy, self.dy, n, ptr(self.sums), ptr(self.gram),
                                         ptr(scratch(nb, x.device)), nb, stream_ptr(x.device)), "moments_accumulate")
        self.count += n
        return self

    def state(self):
        """(n, sx, sy, Sxx, Sxy, Syy) as host float64 numpy arrays (sy, Sxy, Syy empty in the one-stream form)."""
        s = self.sums.cpu().numpy()
        g = self.gram.cpu().numpy()
        dx = self.dx
        return (self.count, s[:dx].copy(), s[dx:].copy(), g[:dx, :dx].copy(), g[:dx, dx:].copy(), g[dx:, dx:].copy())


# --------------------------------------------------------------------------- the solve, on the host
def _pinv_psd(g):
    """Pseudo-inverse of a symmetric positive semi-definite matrix from its eigen-decomposition, keeping the eigenvalues
    above lambda_max * 1e6 * eps."""
    lam, vec = np.linalg.eigh(g)
    top = lam[-1] if lam.size else 0.0
    keep = lam > top * 1e6 * _EPS
    if top <= 0.0 or not keep.any():
        return np.zeros_like(g)
    v = vec[:, keep]
    return (v / lam[keep]) @ v.T


def _pinv_general(a):
    """numpy's pinv with scipy.linalg.pinv's default cut-off (max(shape) * eps), which sklearn uses for the rotations."""
    return np.linalg.pinv(a, rcond=max(a.shape) * _EPS)


def _centre_scale(n, s, S):
    """Centred Gram matrix pieces: mean, unbiased standard deviation (0 -> 1) of the columns with sum s and raw squares diag(S).
    A centred square below the rounding noise of the subtraction counts as zero: a constant column, whose variance sklearn
    finds exactly zero on the data."""
    mean = s / n
    css = np.diag(S) - s * s / n
    css = np.where(css <= 8.0 * n * _EPS * np.abs(np.diag(S)), 0.0, css)
    std = np.sqrt(css / (n - 1)) if n > 1 else np.zeros_like(css)
    std = np.where(std == 0.0, 1.0, std)
    return mean, std, css == 0.0


def cca_from_moments(n, sx, sy, Sxx, Sxy, Syy, n_components, max_iter=500, tol=1e-06):
    """sklearn.cross_decomposition.CCA(n_components, scale=True, max_iter, tol).fit(X, Y) from the second moments of X and Y:
    the count n, the column sums sx, sy and the raw products Sxx = X^T X, Sxy = X^T Y, Syy = Y^T Y.  Returns a CCAModel.

    It restates sklearn's _PLS.fit (NIPALS, mode B, norm_y_weights, canonical deflation) in covariance space.  With the
    centred, scaled data Xk, Yk and Gxx = Xk^T Xk, Gxy = Xk^T Yk, Gyy = Yk^T Yk, the power iteration on a y weight vector c
    (y_score = Yk c) is  w = Gxx^+ Gxy c, normalised;  v = Gyy^+ Gyx w, normalised;  c = v / (v.v + eps);  the loadings are
    p = Gxx w / (w^T Gxx w), q = Gyy v / (v^T Gyy v), and the deflation of Xk, Yk by their scores is rank one on each G.

    One deliberate deviation: the pseudo-inverses come from eigh of Gxx, Gyy keeping eigenvalues lambda > lambda_max * 1e6 * eps,
    where sklearn keeps singular values of the DATA s > s_max * 1e6 * eps (lambda = s^2).  In covariance space sklearn's
    cut-off lies below the rounding noise of a deflated direction (sqrt(eps) * s_max), and with it components after the
    first do not converge.  The two differ only for data whose condition number exceeds about 6e4.  Likewise a column whose centred
    sum of squares, or a y column whose deflated one, is within rounding of zero is treated as constant (sklearn tests the entries
    of the data against 10 eps)."""
    n = int(n)
    sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
    Sxx, Sxy, Syy = (np.asarray(a, np.float64) for a in (Sxx, Sxy, Syy))
    p, q = sx.shape[0], sy.shape[0]
    if Sxx.shape != (p, p) or Sxy.shape != (p, q) or Syy.shape != (q, q):
        raise ValueError(f"cca_from_moments: shapes {Sxx.shape}, {Sxy.shape}, {Syy.shape} do not fit sums of {p} and {q}")
    if n < 2:
        raise ValueError(f"cca_from_moments: {n} sample(s); at least 2 are required")
    bound = min(n, p, q)
    if n_components > bound:
        raise ValueError(f"`n_components` upper bound is {bound}. Got {n_components} instead. Reduce `n_components`.")

    x_mean, x_std, x_const = _centre_scale(n, sx, Sxx)
    y_mean, y_std, y_const = _centre_scale(n, sy, Syy)
    Gxx = (Sxx - np.outer(sx, sx) / n) / np.outer(x_std, x_std)
    Gyy = (Syy - np.outer(sy, sy) / n) / np.outer(y_std, y_std)
    Gxy = (Sxy - np.outer(sx, sy) / n) / np.outer(x_std, y_std)
    Gxx[x_const, :] = 0.0
    Gxx[:, x_const] = 0.0
    Gxy[x_const, :] = 0.0
    Gyy[y_const, :] = 0.0
    Gyy[:, y_const] = 0.0
    Gxy[:, y_const] = 0.0

    gyy0 = np.diag(Gyy).copy()
    W = np.zeros((p, n_components))
    V = np.zeros((q, n_components))
    P = np.zeros((p, n_components))
    Q = np.zeros((q, n_components))
    n_iter = []
    for k in range(n_components):
        # (sklearn zeroes the y columns whose every entry is below 10 eps; the start is the first column with an entry above eps.
        #  Here a residual sum of squares cannot be told from zero below the rounding of its deflation, 64 eps of the column's own)
        dead = np.diag(Gyy) <= np.maximum(n * (10 * _EPS) ** 2, 64 * _EPS * gyy0)
        Gyy[dead, :] = 0.0
        Gyy[:, dead] = 0.0
        Gxy[:, dead] = 0.0
        alive = np.flatnonzero(np.diag(Gyy) > 0.0)
        if alive.size == 0:
            warnings.warn(f"y residual is constant at iteration {k}")
            break
        c = np.zeros(q)
        c[alive[0]] = 1.0
        Pxx, Pyy = _pinv_psd(Gxx), _pinv_psd(Gyy)
        Mx, My = Pxx @ Gxy, Pyy @ Gxy.T
        w_old = 100.0
        for i in range(max_iter):
            w = Mx @ c
            w /= np.sqrt(w @ w) + _EPS
            v = My @ w
            v /= np.sqrt(v @ v) + _EPS
            c = v / (v @ v + _EPS)
            diff = w - w_old
            if diff @ diff < tol or q == 1:
                break
            w_old = w
        n_iter.append(i + 1)
        if i + 1 == max_iter:
            warnings.warn("Maximum number of iterations reached")
        sign = np.sign(w[np.argmax(np.abs(w))])
        w = w * sign
        v = v * sign
        gw, gv = Gxx @ w, Gyy @ v
        tt, uu = w @ gw, v @ gv
        pk, qk = gw / tt, gv / uu
        gxy_v, gyx_w = Gxy @ v, Gxy.T @ w
        tu = w @ gxy_v
        Gxy -= np.outer(pk, gyx_w) + np.outer(gxy_v, qk) - tu * np.outer(pk, qk)
        Gxx -= tt * np.outer(pk, pk)
        Gyy -= uu * np.outer(qk, qk)
        W[:, k], V[:, k], P[:, k], Q[:, k] = w, v, pk, qk

    x_rot = W @ _pinv_general(P.T @ W)
    y_rot = V @ _pinv_general(Q.T @ V)
    coef = x_rot @ Q.T
    coef = (coef * y_std).T / x_std
    return CCAModel(dict(x_weights_=W, y_weights_=V, x_loadings_=P, y_loadings_=Q, x_rotations_=x_rot, y_rotations_=y_rot,
                         coef_=coef, intercept_=y_mean.copy(), n_iter_=np.asarray(n_iter, np.int64), _x_mean=x_mean,
                         _y_mean=y_mean, _x_std=x_std, _y_std=y_std),
                    n_samples=n, moments=dict(sx=sx, sy=sy, Sxx=Sxx, Sxy=Sxy, Syy=Syy))


# --------------------------------------------------------------------------- the fitted model
ATTRIBUTES = ("x_weights_", "y_weights_", "x_loadings_", "y_loadings_", "x_rotations_", "y_rotations_", "coef_", "intercept_",
              "n_iter_", "_x_mean", "_y_mean", "_x_std", "_y_std")
_MOMENTS = ("sx", "sy", "Sxx", "Sxy", "Syy")


class CCAModel:
    """The fitted attributes of sklearn's CCA under its names, n_samples_, and the raw moments they were fitted on."""

    def __init__(self, attributes, n_samples, moments=None):
        for name in ATTRIBUTES:
            setattr(self, name, np.asarray(attributes[name]))
        self.n_samples_ = int(n_samples)
        self.moments_ = None if moments is None else {k: np.asarray(moments[k], np.float64) for k in _MOMENTS}
        self._affine = {}

    @property
    def n_components(self):
        return self.x_rotations_.shape[1]

    def _projection(self, side, device):
        """((X - mean) / std) @ rotations as one affine map: weight [n_components, d] and bias, folded in f64 on the host."""
        key = (side, str(device))
        if key not in self._affine:
            mean, std, rot = ((self._x_mean, self._x_std, self.x_rotations_) if side == "x" else
                              (self._y_mean, self._y_std, self.y_rotations_))
            weight = (rot / std[:, None]).T
            bias = -(mean / std) @ rot
            self._affine[key] = (torch.from_numpy(np.ascontiguousarray(weight, np.float32)).to(device),
                                 torch.from_numpy(np.ascontiguousarray(bias, np.float32)).to(device))
        return self._affine[key]

    def _project(self, t, side):
        weight, bias = self._projection(side, t.device)
        k = weight.shape[1]
        if t.dtype != torch.float32:
            raise TypeError(f"cpc2_amd kernels are fp32 only (got {t.dtype})")
        if t.shape[-1] != k:
            raise ValueError(f"transform: expected a last dimension of {k}, got {tuple(t.shape)}")
        t2 = t.contiguous().reshape(-1, k)
        m, nc = t2.shape[0], weight.shape[0]
        out = torch.empty(m, nc, dtype=torch.float32, device=t.device)
        if m:
            check(_lib.load().cpc_gemm_nt(ptr(t2), k, ptr(weight), k, ptr(out), nc, ptr(bias), m, nc, k, stream_ptr(t.device)),
                  "gemm_nt")
        return out.view(*t.shape[:-1], nc)

    def transform(self, X, Y=None):
        """sklearn's transform on float32 device tensors [..., d]: x scores, or (x scores, y scores) with Y."""
        require_gpu(X, Y)
        xs = self._project(X, "x")
        return xs if Y is None else (xs, self._project(Y, "y"))

    def save(self, path):
        arrays = {name: getattr(self, name) for name in ATTRIBUTES}
        arrays["n_samples_"] = np.asarray(self.n_samples_, np.int64)
        if self.moments_ is not None:
            arrays.update(self.moments_)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            moments = {k: z[k] for k in _MOMENTS} if all(k in z.files for k in _MOMENTS) else None
            return cls({name: z[name] for name in ATTRIBUTES}, int(z["n_samples_"]), moments)


def to_sklearn(model):
    """A sklearn.cross_decomposition.CCA carrying the fitted attributes of `model`, so that its pickle transforms as the
    reference's output file does."""
    try:
        from sklearn.cross_decomposition import CCA
    except ImportError as e:
        raise ImportError("scikit-learn is not installed: the fitted model is in the .npz file written by CCAModel.save "
                          "(cpc2_amd.cca.CCAModel.load reads it); the .pkl of the reference needs scikit-learn") from e
    cca = CCA(n_components=model.n_components)
    for name in ATTRIBUTES:
        value = getattr(model, name)
        setattr(cca, name, [int(i) for i in value] if name == "n_iter_" else np.array(value, np.float64))
    cca.n_features_in_ = model.x_rotations_.shape[0]
    cca._n_features_out = model.n_components
    cca._norm_y_weights = True
    cca._predict_1d = False
    return cca
