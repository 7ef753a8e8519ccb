#!/usr/bin/env python3
"""k-means kernels on one MI355X (csrc/kmeans.hip).  Writes profiles/kmeans_bench.json (and prints it).

Sizes: every (k, batchSizeGPU) pair of the reference's docs table (64 frames per 10240-sample window) at d = 256 and 512,
and n = 32000 at every k.  For each size:
  assign_ms / assign_valu_floor_frac   kmeans_assign_kernel against the VALU floor: 2 n k d lane-instructions (one v_sub
                                       + one v_fmac per term) at 78.6 T lane-instructions/s (157.3 TFLOP/s f32 FMA / 2)
  accumulate_ms / accumulate_GBps      bytes moved: x read twice (partial pass + index reads), sums read + written
  step_ms / torch_step_ms              kMeanClusterStep per batch against a plain-torch baseline (broadcast distance in
                                       chunks of at most 1 GiB, argmin, index_add_), run alternately in the same process
Then one kMeanGPU iteration with CPC-small on synthetic audio (500 windows x 10240 samples), split into featureMaker and
clustering time.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/kmeans_bench.py` apart.

    python tools/kmeans_bench.py [--reps 20] [--no-iteration]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd.clustering import clustering as C  # noqa: E402

TABLE = [(20, 500), (50, 500), (100, 300), (200, 200), (500, 100), (2000, 50)]
LANE_OPS_PER_S = 157.3e12 / 2
HBM_BPS = 8.0e12
DEV = torch.device("cuda:0")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / reps


def torch_step(x, ck):
    """Plain-torch baseline: broadcast distances, argmin, index_add_ sums and bincount."""
    k = ck.size(0)
    rows = max(1, (1 << 28) // (k * ck.size(1)))                      # broadcast chunks of at most 1 GiB
    index = torch.cat([((x[i:i + rows, None, :] - ck[None]) ** 2).sum(dim=2).argmin(dim=1)
                       for i in range(0, x.size(0), rows)])
    sums = torch.zeros_like(ck).index_add_(0, index, x)
    return sums, torch.bincount(index, minlength=k)


def size_record(n, d, k, reps):
    gen = torch.Generator().manual_seed(n + d + k)
    x = torch.randn(n, d, generator=gen).to(DEV)
    ck = torch.randn(k, d, generator=gen).to(DEV)
    index, _ = C.kmeans_assign(x, ck, want_min_sq=False)
    sums = torch.zeros(k, d, device=DEV)
    counts = torch.zeros(k, dtype=torch.long, device=DEV)
    assign_ms = timed(lambda: C.kmeans_assign(x, ck, want_min_sq=False), reps)
    acc_ms = timed(lambda: C.kmeans_accumulate(x, index, sums, counts), reps)
    step = C.kMeanClusterStep(k, d).to(DEV)
    step.Ck.copy_(ck.view(1, k, d))
    xs = x.view(n, 1, d)
    rec = dict(n=n, d=d, k=k, assign_ms=assign_ms,
               assign_valu_floor_frac=(2.0 * n * k * d / LANE_OPS_PER_S) / (assign_ms / 1e3),
               accumulate_ms=acc_ms, accumulate_GBps=(2 * n * d * 4 + 2 * k * d * 4 + n * 4) / (acc_ms / 1e3) / 1e9)
    rec["accumulate_hbm_frac"] = rec["accumulate_GBps"] * 1e9 / HBM_BPS
    # the two step implementations alternately, 3 rounds, best of each
    mine, base = [], []
    for _ in range(3):
        mine.append(timed(lambda: step(xs), reps))
        base.append(timed(lambda: torch_step(x, ck), max(1, reps // 4)))
    rec.update(step_ms=min(mine), torch_step_ms=min(base), speedup=min(base) / min(mine))
    return rec


def iteration_record(k=50, windows=500):
    """One kMeanGPU-style pass over 500 windows of synthetic audio with CPC-small (hidden 256), one batch."""
    from cpc2_amd.model import CPCAR, CPCEncoder, CPCModel
    from cpc2_amd.feature_loader import FeatureModule
    torch.manual_seed(0)
    model = CPCModel(CPCEncoder(256), CPCAR(256, 256, False, 1)).to(DEV).eval()
    fm = FeatureModule(model, False)
    wave = (0.1 * torch.randn(windows, 1, 10240)).to(DEV)
    step = C.kMeanClusterStep(k, 256).to(DEV)
    with torch.no_grad():
        feats = fm((wave, None))
        step.Ck.copy_(feats.reshape(-1, 256)[:k].view(1, k, 256))
        Ck1 = torch.zeros(1, k, 256, device=DEV)
        nItems = torch.zeros(k, dtype=torch.long, device=DEV)
        fm_ms = timed(lambda: fm((wave, None)), 5)
        cl_ms = timed(lambda: step.accumulate(feats.view(-1, 1, 256), Ck1, nItems), 5)
    return dict(windows=windows, k=k, frames=int(feats.shape[0] * feats.shape[1]), featureMaker_ms=fm_ms,
                clustering_ms=cl_ms, clustering_share=cl_ms / (fm_ms + cl_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-iteration", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.json"))
    a = ap.parse_args()
    sizes = [(b * 64, d, k) for d in (256, 512) for k, b in TABLE] + [(32000, 512, k) for k, _ in TABLE]
    out = dict(device=torch.cuda.get_device_name(0), sizes=[])
    t0 = time.perf_counter()
    for n, d, k in sizes:
        out["sizes"].append(size_record(n, d, k, a.reps))
    if not a.no_iteration:
        out["iteration"] = iteration_record()
    out["wall_s"] = time.perf_counter() - t0
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
