"""Writes tests/golden/g29_dim_reduction.npz by running the REFERENCE's cpc/criterion/research/dim_reduction.py (PCA, SFALinear)
on the CPU in float64, on float32 inputs that are recorded with the results.

    CPC_REFERENCE=DIR PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dim_reduction.py

The reference is imported unmodified; progressbar is stubbed, and torch.symeig -- removed from torch -- is mapped to
torch.linalg.eigh in this process only (same eigenvalue order; the sign of an eigenvector is LAPACK's).  Arrays only.

Cases k = 8 on 3 windows of 16 frames and k = 64 on 6 windows of 40 frames (tests/dim_reduction_oracle.ar1_features: an AR(1)
latent with a time constant per dimension, mixed by a random matrix, plus an offset, on a grid of 2^-10 so that the raw sums are
exact in f64), with two more windows of the same process held out.  Recorded per case: the inputs; the raw buffers after update
and N, N_x, N_speed; every buffer after build; forward of the held-out windows for PCA and SFALinear, and for SFALinear after
selectDimensions(the slower half of the directions).

The maker FAILS -- change the seed, not a limit -- when the smallest relative eigenvalue gap of a case is below 1e-4, or when the
numpy statement of tests/dim_reduction_oracle.py is not within 1e-8 of the reference (eigenvector rows compared after the sign
rule, each buffer relative to its largest magnitude).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CPC_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "cpc")):
    raise SystemExit("set CPC_REFERENCE to a checkout of the reference repository (the directory that holds cpc/)")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.modules["progressbar"] = types.ModuleType("progressbar")
torch.symeig = lambda a, eigenvectors=True: torch.linalg.eigh(a)        # (torch keeps the name as a stub that raises)
_spec = importlib.util.spec_from_file_location("ref_dim_reduction",
                                               os.path.join(REF, "cpc", "criterion", "research", "dim_reduction.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

import dim_reduction_oracle as DO      # noqa: E402

CASES = [("k8", 3, 16, 8), ("k64", 6, 40, 64)]      # tag, windows, frames, k
HELD_OUT = 2
MIN_GAP = 1e-4
LIMIT = 1e-8
SIGNED = ("PCA_mul", "projection")


def buffers(module):
    return {k: v.detach().numpy().astype(np.float64).copy() for k, v in module.state_dict().items()}


def deviation(mine, theirs):
    worst = 0.0
    for name, value in theirs.items():
        a, b = np.asarray(mine[name], np.float64), np.asarray(value, np.float64)
        if name in SIGNED:
            a, b = DO.sign_rule(a[0]), DO.sign_rule(b[0])
        worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=33)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g29_dim_reduction.npz"))
    args = ap.parse_args(argv)
    out = {"seed": np.asarray(args.seed), "tags": np.asarray([c[0] for c in CASES])}
    for i, (tag, b, s, k) in enumerate(CASES):
        data = DO.ar1_features(b + HELD_OUT, s, k, args.seed + i)
        x, held = data[:b], data[b:]
        out[f"{tag}_x"], out[f"{tag}_held_out"] = x, held

        pca = ref.PCA(k).double()
        pca.update(torch.from_numpy(x).double())
        raw = buffers(pca)
        out[f"{tag}_pca_raw_var"], out[f"{tag}_pca_raw_mean"], out[f"{tag}_pca_N"] = raw["var"], raw["mean"], np.asarray(pca.N)
        pca.build()
        built = buffers(pca)
        for name, value in built.items():
            out[f"{tag}_pca_{name}"] = value
        out[f"{tag}_pca_forward"] = pca(torch.from_numpy(held).double().clone()).numpy()
        mine = DO.pca_build(raw["mean"], raw["var"], pca.N)
        dev_pca, gap_pca = deviation(mine, built), DO.relative_gap(built["PCA_values"])

        sfa = ref.SFALinear(k).double()
        sfa.update(torch.from_numpy(x).double())
        raw = buffers(sfa)
        for name in ("covar_speed", "mean_x", "square_x", "covar_x"):
            out[f"{tag}_sfa_raw_{name}"] = raw[name]
        out[f"{tag}_sfa_N_x"], out[f"{tag}_sfa_N_speed"] = np.asarray(sfa.N_x), np.asarray(sfa.N_speed)
        if (sfa.N_x, sfa.N_speed) != DO.counts(b, s, exact=False):
            raise SystemExit(f"case {tag}: the reference counts {sfa.N_x}, {sfa.N_speed}, the statement {DO.counts(b, s, False)}")
        if not np.array_equal(raw["square_x"], np.diag(raw["covar_x"])):
            raise SystemExit(f"case {tag}: the raw square_x is not the diagonal of the raw covar_x")
        sfa.build()
        built = buffers(sfa)
        for name, value in built.items():
            out[f"{tag}_sfa_{name}"] = value
        out[f"{tag}_sfa_forward"] = sfa(torch.from_numpy(held).double().clone()).numpy()
        select = (torch.arange(k) < k // 2).long()              # the slower half: eigenvalues ascend
        sfa.selectDimensions(select)
        out[f"{tag}_sfa_select"] = select.numpy()
        out[f"{tag}_sfa_forward_selected"] = sfa(torch.from_numpy(held).double().clone()).numpy()
        mine = DO.sfa_build(raw["mean_x"], raw["covar_x"], raw["covar_speed"], sfa.N_x, sfa.N_speed)
        dev_sfa, gap_sfa = deviation(mine, built), DO.relative_gap(built["PCA_values"])
        fwd = np.abs(DO.sfa_forward(built, held) - out[f"{tag}_sfa_forward"]).max()

        print(f"case {tag}: PCA deviation {dev_pca:.2e} gap {gap_pca:.2e}; SFA deviation {dev_sfa:.2e} gap {gap_sfa:.2e}; "
              f"SFA forward statement {fwd:.2e}")
        if min(gap_pca, gap_sfa) < MIN_GAP:
            raise SystemExit(f"case {tag}: relative eigenvalue gap below {MIN_GAP:g}; change the seed")
        if not max(dev_pca, dev_sfa) <= LIMIT:
            raise SystemExit(f"case {tag}: the numpy statement deviates by more than {LIMIT:g}; change the seed")
        out[f"{tag}_deviation"] = np.asarray(max(dev_pca, dev_sfa))
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {size} bytes")
    if size >= 1 << 20:
        raise SystemExit("the golden file must stay under 1 MiB")


if __name__ == "__main__":
    main(sys.argv[1:])
