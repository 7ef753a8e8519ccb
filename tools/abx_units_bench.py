#!/usr/bin/env python3
"""ABX on quantized units on one MI355X: the unit path (ABXUnitLoader + cpc_abx_dtw_units) against the dense path on the
one-hot features (ABXFeatureLoader + cpc_abx_dtw), on the same triplets of a seeded synthetic item set shaped like a
ZeroSpeech ABX task (tools/abx_bench.py's: 20 000 items of 3-25 frames), units drawn in runs of 1-5 frames.

For every n_units and for within / across: host planning, batched scoring of both paths (alternated in one process, after
a warm-up of every shape), unique pairs, DTW cells, the time spent inside the DTW calls (device events around _dtw_pairs:
list upload + kernel), peak device memory of both, and an fp64 check (tests/abx_oracle.py) of a sample of the timed
triplets, which must be EQUAL for the cosine distance.  The dense path is skipped where its matrix exceeds --dense_max_gb.
Prints one JSON line (and writes it to --out).

    python tools/abx_units_bench.py [--n_units 50 200 2000] [--out profiles/abx_units_bench.json]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/abx_units_bench.py --n_units N --repeats 1`
separately, one n_units per run (abx_dtw_kernel's time depends on it, abx_dtw_units_kernel's must not).
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
from cpc2_amd.eval.eval_ABX_clustering import one_hot  # noqa: E402
from tests import abx_oracle as O  # noqa: E402

COS = abx_g.get_cosine_distance_batch


def item_set(a, path):
    """Item file and per-file frame counts: `files_per_speaker` files per speaker, items of 3-25 frames back to back."""
    rng = np.random.default_rng(a.seed)
    n_files = a.speakers * a.files_per_speaker
    per_file = -(-a.items // n_files)
    ctx = [(f"c{i}", f"d{i}") for i in range(a.contexts)]
    lines, frames = ["#file onset offset #phone prev-phone next-phone speaker"], {}
    for f in range(n_files):
        spk = f % a.speakers
        lens = rng.integers(3, 26, per_file)
        t = 1
        for n in lens:
            p = int(rng.integers(0, a.phones))
            c = ctx[int(rng.integers(0, a.contexts))]
            lines.append(f"f{f} {(t + 0.3) / 100:.4f} {(t + n + 0.7) / 100:.4f} p{p} {c[0]} {c[1]} s{spk}")
            t += int(n)
        frames[f"f{f}"] = int(lens.sum()) + 2
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return frames


def unit_runs(rng, n, n_units):
    out = np.repeat(rng.integers(0, n_units, n), rng.integers(1, 6, n))
    return torch.from_numpy(out[:n].astype(np.int64))


def timed(fn):
    """(result, wall seconds, seconds between device events around the _dtw_pairs calls inside fn)."""
    spans = []
    real = abx_g._dtw_pairs

    def wrapped(items, px, py, code):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real(items, px, py, code)
        e1.record()
        spans.append((e0, e1))
        return out

    torch.cuda.synchronize()
    abx_g._dtw_pairs = wrapped
    t0 = time.perf_counter()
    try:
        out = fn()
    finally:
        abx_g._dtw_pairs = real
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, sum(e0.elapsed_time(e1) for e0, e1 in spans) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_units", type=int, nargs="+", default=[50, 200, 2000])
    ap.add_argument("--speakers", type=int, default=40)
    ap.add_argument("--phones", type=int, default=40)
    ap.add_argument("--contexts", type=int, default=3)
    ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--files_per_speaker", type=int, default=5)
    ap.add_argument("--max_size_group", type=int, default=10)
    ap.add_argument("--max_x_across", type=int, default=5)
    ap.add_argument("--oracle_sample", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--dense_max_gb", type=float, default=8.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()

    tmp = tempfile.mkdtemp(prefix="abx_units_bench_")
    item_path = os.path.join(tmp, "bench.item")
    frames = item_set(a, item_path)
    seqs = [(k, k) for k in frames]
    dev = torch.device("cuda:0")
    res = {"workload": {k: getattr(a, k) for k in ("speakers", "phones", "contexts", "items", "max_size_group",
                                                   "max_x_across", "seed")}, "runs": []}
    for n_units in a.n_units:
        rng = np.random.default_rng(a.seed + n_units)
        units = {k: unit_runs(rng, n, n_units) for k, n in frames.items()}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        uds = abx_it.ABXUnitLoader(item_path, seqs, lambda p: units[p], 100.0, True, n_units)
        uitems = abx_g._UnitItems(*uds.device_units(dev), [f[1] for f in uds.features],
                                  {abx_g.COSINE: abx_g.unit_frame_distances(n_units, True, COS)})
        torch.cuda.synchronize()
        r = {"n_units": n_units, "n_items": len(uds), "frames": int(uds.units.numel()),
             "unit_load_upload_s": round(time.perf_counter() - t0, 3)}
        dense_bytes = uds.units.numel() * (-(-(n_units + 1) // 4) * 4) * 4
        r["dense_matrix_bytes"] = int(dense_bytes)
        ditems = dds = None
        if dense_bytes <= a.dense_max_gb * 2 ** 30:
            t0 = time.perf_counter()
            dds = abx_it.ABXFeatureLoader(item_path, seqs, lambda p: one_hot(units[p], n_units).unsqueeze(0), 100.0, True)
            dp = -(-dds.feature_dim // 4) * 4
            ditems = abx_g._Items(*dds.device_frames(dev, dp), [f[1] for f in dds.features])
            torch.cuda.synchronize()
            r["dense_load_upload_s"] = round(time.perf_counter() - t0, 3)
            assert dds.features == uds.features
        random.seed(a.seed)
        peak = {"units": 0, "dense": 0}
        for mode in ("within", "across"):
            it = uds.get_iterator(mode, a.max_size_group, a.max_x_across)
            t0 = time.perf_counter()
            _coords, trips = abx_g.plan_triplets(it)
            m = {"triplets": len(trips), "plan_s": round(time.perf_counter() - t0, 3)}
            paths = [("units", uitems)] + ([("dense", ditems)] if ditems is not None else [])
            for name, items in paths:                              # warm-up: every shape, both paths
                abx_g._score_triplets(items, trips, it.symmetric, abx_g.COSINE)
            walls = {name: [] for name, _ in paths}
            dtws = {name: [] for name, _ in paths}
            thetas = {}
            for _rep in range(a.repeats):                          # alternate the two paths
                for name, items in paths:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    stats = {}
                    theta, wall, dtw_s = timed(lambda: abx_g._score_triplets(items, trips, it.symmetric, abx_g.COSINE,
                                                                             stats=stats))
                    peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - before)
                    walls[name].append(round(wall, 4))
                    dtws[name].append(round(dtw_s, 5))
                    thetas[name] = theta
            m.update({"unique_pairs": stats["unique_pairs"], "chunks": stats["chunks"], "dtw_cells": stats["dtw_cells"]})
            for name, _ in paths:
                m[f"{name}_score_wall_s"] = walls[name]
                m[f"{name}_dtw_call_s"] = dtws[name]
                m[f"{name}_dtw_cells_per_s"] = round(stats["dtw_cells"] / min(dtws[name]), 1)
            if ditems is not None:
                m["theta_equal"] = bool(torch.equal(thetas["units"], thetas["dense"]))
                m["dtw_call_ratio_dense_over_units"] = round(min(dtws["dense"]) / min(dtws["units"]), 2)
            # fp64 oracle on a sample of the timed triplets: equal, not close (every cost is a multiple of 0.5)
            seq = [uds.units[f[0]:f[0] + f[1]].numpy() for f in uds.features]
            cache = {}

            def dtw(i, j):
                if (i, j) not in cache:
                    cache[i, j] = O.dtw(np.where(seq[i][:, None] == seq[j][None, :], 0.0, 0.5))[0]
                return cache[i, j]

            sample = sorted(random.Random(a.seed + 1).sample(range(len(trips)), min(a.oracle_sample, len(trips))))
            equal = 0
            for i in sample:
                ta, tb, tx = trips[i]
                dxb = np.array([[dtw(p, q) for q in tb] for p in tx])
                if it.symmetric:
                    dxa = np.array([[np.nan if p == q else dtw(tx[min(p, q)], ta[max(p, q)]) for q in range(len(ta))]
                                    for p in range(len(tx))])
                else:
                    dxa = np.array([[dtw(p, q) for q in ta] for p in tx])
                lt, eq, _ = O.counts(dxa, dxb)
                t64 = lambda v: torch.tensor([v], dtype=torch.int64)  # noqa: E731
                want = abx_g.theta_from_counts(t64(lt), t64(eq), t64(len(ta)), t64(len(tb)), t64(len(tx)), it.symmetric)
                equal += int(want[0] == thetas["units"][i])
            m["oracle_checked"], m["oracle_equal"] = len(sample), equal
            r[mode] = m
        # what a path keeps on the device (its items) plus the most a scoring call adds to it (lists, pair results)
        resident = {"units": sum(t.numel() * t.element_size() for t in (uitems.units, uitems.off, uitems.lens))}
        if ditems is not None:
            resident["dense"] = sum(t.numel() * t.element_size() for t in (ditems.frames, ditems.off, ditems.lens))
        r["resident_device_bytes"] = {k: int(v) for k, v in resident.items()}
        r["peak_device_bytes"] = {k: int(resident[k] + peak[k]) for k in resident}
        r["resident_device_bytes_after"] = int(torch.cuda.memory_allocated() - base)
        res["runs"].append(r)
        del uitems, ditems, uds, dds
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
