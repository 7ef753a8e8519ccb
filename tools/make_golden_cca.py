"""Writes tests/golden/g28_cca.npz: sklearn.cross_decomposition.CCA on the CPU, on three synthetic problems recorded with their
float32 inputs.   python tools/make_golden_cca.py [--seed 7]

Each problem has r shared latents with correlations linspace(0.95, 0.2, r), the remaining columns are noise, each side is mixed by
(randn + 3 I) and shifted by +3 (X) / -1 (Y).  Recorded per problem: the inputs, every fitted attribute, n_iter_, transform(X, Y),
and the largest deviation of cpc2_amd.cca.cca_from_moments (on numpy float64 moments of the same inputs) from sklearn, relative to
each attribute's largest magnitude.

The maker FAILS -- change the seed, not a limit -- unless: no ConvergenceWarning was raised, every n_iter_ is below 100,
cca_from_moments gives the same n_iter_, and every attribute is within 1e-9 of sklearn's.
"""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBLEMS = [("a", 3000, 12, 10, 6, 4), ("b", 2000, 24, 16, 8, 5), ("c", 257, 3, 1, 1, 1)]     # tag, n, p, q, latents, components
ATTRIBUTES = ("x_weights_", "y_weights_", "x_loadings_", "y_loadings_", "x_rotations_", "y_rotations_", "coef_", "intercept_",
              "_x_mean", "_y_mean", "_x_std", "_y_std")
MAX_ITER_SEEN = 100
LIMIT = 1e-9


def make_problem(rng, n, p, q, r):
    rho = np.linspace(0.95, 0.2, r)
    z = rng.standard_normal((n, r))
    zx = z
    zy = rho * z + np.sqrt(1.0 - rho ** 2) * rng.standard_normal((n, r))
    x0 = np.concatenate([zx, rng.standard_normal((n, p - r))], axis=1)
    y0 = np.concatenate([zy, rng.standard_normal((n, q - r))], axis=1)
    x = x0 @ (rng.standard_normal((p, p)) + 3.0 * np.eye(p)) + 3.0
    y = y0 @ (rng.standard_normal((q, q)) + 3.0 * np.eye(q)) - 1.0
    return x.astype(np.float32), y.astype(np.float32)


def main(argv):
    from sklearn.cross_decomposition import CCA
    from sklearn.exceptions import ConvergenceWarning

    from cpc2_amd.cca import cca_from_moments

    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g28_cca.npz"))
    args = ap.parse_args(argv)
    rng = np.random.default_rng(args.seed)
    out = {"seed": np.asarray(args.seed), "tags": np.asarray([t[0] for t in PROBLEMS])}
    for tag, n, p, q, r, nc in PROBLEMS:
        X, Y = make_problem(rng, n, p, q, r)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            cca = CCA(n_components=nc).fit(X, Y)
            xs, ys = cca.transform(X, Y)
        if any(issubclass(w.category, ConvergenceWarning) for w in caught):
            raise SystemExit(f"problem {tag}: sklearn raised a ConvergenceWarning; change the seed")
        if max(cca.n_iter_) >= MAX_ITER_SEEN:
            raise SystemExit(f"problem {tag}: n_iter_ = {cca.n_iter_} reaches {MAX_ITER_SEEN}; change the seed")
        X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
        model = cca_from_moments(n, X64.sum(0), Y64.sum(0), X64.T @ X64, X64.T @ Y64, Y64.T @ Y64, nc)
        if list(model.n_iter_) != list(cca.n_iter_):
            raise SystemExit(f"problem {tag}: n_iter_ {list(model.n_iter_)} against sklearn's {cca.n_iter_}; change the seed")
        worst = 0.0
        for name in ATTRIBUTES:
            ref = np.asarray(getattr(cca, name), np.float64)
            worst = max(worst, float(np.abs(getattr(model, name) - ref).max() / np.abs(ref).max()))
        print(f"problem {tag}: n={n} p={p} q={q} components={nc} n_iter_={cca.n_iter_} deviation {worst:.2e}")
        if not worst <= LIMIT:
            raise SystemExit(f"problem {tag}: deviation {worst:.2e} above {LIMIT:g}; change the seed")
        out[f"{tag}_X"], out[f"{tag}_Y"] = X, Y
        out[f"{tag}_n_components"] = np.asarray(nc)
        out[f"{tag}_n_iter_"] = np.asarray(cca.n_iter_, np.int64)
        out[f"{tag}_x_scores"], out[f"{tag}_y_scores"] = xs, ys
        out[f"{tag}_deviation"] = np.asarray(worst)
        for name in ATTRIBUTES:
            out[f"{tag}_{name}"] = np.asarray(getattr(cca, name), np.float64)
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {size} bytes")
    if size >= 1 << 20:
        raise SystemExit("the golden file must stay under 1 MiB")


if __name__ == "__main__":
    main(sys.argv[1:])
