#!/usr/bin/env python3
"""ABX scoring throughput on one MI355X: a seeded synthetic phone-level item set shaped like a ZeroSpeech ABX task,
scored by the batched kernels (get_abx_scores_dtw_on_group) and, alternated with it in the same process, by the
reference-shaped path (one get_theta_group_dtw per triplet, same kernels) on a sample of the triplets.  Prints one JSON
line.  An fp64 oracle (tests/abx_oracle.py) checks a sample of the timed triplets.

    python tools/abx_bench.py [--speakers 40 --phones 40 --items 20000 --dim 256 --max_size_group 10 --max_x_across 5]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/abx_bench.py ...` separately.
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd.eval.ABX import abx_group_computation as abx_g  # noqa: E402
from cpc2_amd.eval.ABX import abx_iterators as abx_it  # noqa: E402
from tests import abx_oracle as O  # noqa: E402


def workload(a, path):
    """Item file + per-file features: `files_per_speaker` files per speaker, items of 3-25 frames back to back."""
    rng = np.random.default_rng(a.seed)
    n_files = a.speakers * a.files_per_speaker
    per_file = -(-a.items // n_files)
    pmean = rng.standard_normal((a.phones, a.dim)).astype(np.float32)
    soff = 0.5 * rng.standard_normal((a.speakers, a.dim)).astype(np.float32)
    ctx = [(f"c{i}", f"d{i}") for i in range(a.contexts)]
    lines, feats = ["#file onset offset #phone prev-phone next-phone speaker"], {}
    for f in range(n_files):
        spk = f % a.speakers
        lens = rng.integers(3, 26, per_file)
        total = int(lens.sum()) + 2
        x = 1.2 * rng.standard_normal((total, a.dim)).astype(np.float32)
        t = 1
        for n in lens:
            p = int(rng.integers(0, a.phones))
            c = ctx[int(rng.integers(0, a.contexts))]
            x[t:t + n] += pmean[p] + soff[spk]
            # onset / offset in seconds such that the reference's slicing gives frames t .. t+n-1
            lines.append(f"f{f} {(t + 0.3) / 100:.4f} {(t + n + 0.7) / 100:.4f} p{p} {c[0]} {c[1]} s{spk}")
            t += int(n)
        feats[f"f{f}"] = torch.from_numpy(x)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return feats


def timed(fn):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    out = fn()
    ev1.record()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, ev0.elapsed_time(ev1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, default=40)
    ap.add_argument("--phones", type=int, default=40)
    ap.add_argument("--contexts", type=int, default=3)
    ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--files_per_speaker", type=int, default=5)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--max_size_group", type=int, default=10)
    ap.add_argument("--max_x_across", type=int, default=5)
    ap.add_argument("--per_group_sample", type=int, default=300)
    ap.add_argument("--oracle_sample", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    tmp = tempfile.mkdtemp(prefix="abx_bench_")
    item_path = os.path.join(tmp, "bench.item")
    feats = workload(a, item_path)
    t0 = time.perf_counter()
    ds = abx_it.ABXFeatureLoader(item_path, [(k, k) for k in feats], lambda p: feats[p].clone(), 100.0, True)
    load_s = time.perf_counter() - t0
    dev = torch.device("cuda:0")
    dp = -(-ds.feature_dim // 4) * 4
    (_f, _o, _l), upload_s, _ = timed(lambda: ds.device_frames(dev, dp))
    items = abx_g._Items(*ds.device_frames(dev, dp), [f[1] for f in ds.features])
    cos = abx_g.get_cosine_distance_batch
    res = {"workload": {k: getattr(a, k) for k in ("speakers", "phones", "contexts", "items", "dim", "max_size_group",
                                                   "max_x_across", "seed")},
           "n_items": len(ds), "frames": int(ds.data.size(0)), "feature_dim": ds.feature_dim, "dp": dp,
           "load_s": round(load_s, 3), "upload_s": round(upload_s, 4)}
    random.seed(a.seed)
    for mode in ("within", "across"):
        it = ds.get_iterator(mode, a.max_size_group, a.max_x_across)
        t0 = time.perf_counter()
        coords, trips = abx_g.plan_triplets(it)
        plan_s = time.perf_counter() - t0
        r = {"triplets": len(trips), "plan_s": round(plan_s, 3)}
        rng = random.Random(a.seed + 1)
        sample = sorted(rng.sample(range(len(trips)), min(a.per_group_sample, len(trips))))
        batched, pergroup = [], []
        for rep in range(a.repeats):                               # alternate the two paths
            stats = {}
            theta, wall, gpu = timed(lambda: abx_g._score_triplets(items, trips, it.symmetric, abx_g.COSINE, stats=stats))
            batched.append((wall, gpu))

            def per_group():
                out = []
                for i in sample:
                    ta, tb, tx = trips[i]
                    ga, gb, gx = it.group_data(ta), it.group_data(tb), it.group_data(tx)
                    out.append(abx_g.get_theta_group_dtw(ga[0].to(dev), gb[0].to(dev), gx[0].to(dev), ga[1], gb[1], gx[1],
                                                         cos, it.symmetric))
                return out
            pg, pg_wall, _ = timed(per_group)
            pergroup.append(pg_wall)
        assert np.array_equal(np.array(pg, dtype=np.float32), theta.numpy()[sample])
        r.update({"unique_pairs": stats["unique_pairs"], "chunks": stats["chunks"], "dtw_cells": stats["dtw_cells"],
                  "distance_flop": 2 * dp * stats["dtw_cells"],
                  "score_wall_s": [round(w, 4) for w, _ in batched], "score_gpu_event_s": [round(g, 4) for _, g in batched],
                  "per_group_sample": len(sample), "per_group_wall_s": [round(w, 4) for w in pergroup],
                  "per_group_extrapolated_s": round(min(pergroup) / max(1, len(sample)) * len(trips), 2)})
        # fp64 oracle on a sample of the timed triplets
        frames = [ds[i][0].numpy() for i in range(len(ds))]
        worst = 0.0
        for i in sample[:a.oracle_sample]:
            ta, tb, tx = trips[i]
            dxb = O.group_dtw([frames[j] for j in tx], [frames[j] for j in tb], "cosine")
            dxa = O.group_dtw([frames[j] for j in tx], [frames[j] for j in ta], "cosine", symmetric=it.symmetric)
            n_pos = len(ta) * (len(ta) - 1) if it.symmetric else len(ta) * len(tx)
            lo, hi = O.theta_band(dxa, dxb, n_pos * len(tb), 1e-4)
            t = float(theta[i])
            worst = max(worst, lo - t, t - hi)
        r["oracle_checked"] = min(a.oracle_sample, len(sample))
        r["oracle_outside_band"] = round(max(0.0, worst), 8)
        res[mode] = r
    # planning + batched scoring of both modes (best repeat); feature loading and upload listed apart
    res["end_to_end_s"] = round(sum(res[m]["plan_s"] + min(res[m]["score_wall_s"]) for m in ("within", "across")), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
