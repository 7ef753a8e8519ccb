#!/usr/bin/env python3
"""Term detection and term discovery on quantized units on one MI355X (csrc/sdtw_units.hip, csrc/lalign_units.hip; DESIGN.md
section 29): the unit kernels against the dense kernels on the one-hot expansion of the same units, and against cpc_abx_dtw_units.

Workloads: those of tools/term_detection_bench.py (--queries 200 queries of 50..150 frames against --docs 2 000 documents of
300..1 500 frames) and of tools/term_discovery_bench.py (every pair of --utts 360 utterances of 300..1 500 frames), with units
drawn in runs of 1..5 frames from 50, 200 and 2 000 units.  Distances (0, 0.5), the cosine pair; theta 0.25, gamma 0.125.

  kernels   device events around each kernel call, on ONE work list per workload: the unit kernel, cpc_abx_dtw_units (two words
            per cell and no running best: what the third word and the best cost) and the dense kernel on the one-hot rows
            (normalize_with_singularity, cosine), in alternating rounds after a warm-up of all; every round's time is listed with
            the smallest and the spread (max - min) / min.  The unit and the dense outputs are compared bit for bit.
  bytes     the one-hot frames buffer against the units buffer
  tools     python -m cpc2_amd.eval.term_detection / term_discovery from_units on a synthetic hour (--hour_docs 450 documents of
            800 frames with 50 queries cut from them; --utts utterances of 1 000 frames): wall time by stage, from the logs

Prints one JSON line and writes it to --out (default profiles/term_units_bench.json).
    python tools/term_units_bench.py
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd import _lib  # noqa: E402
from cpc2_amd import term_detection as td  # noqa: E402
from cpc2_amd import term_discovery as tdisc  # noqa: E402
from cpc2_amd.eval import term_detection as detection_tool  # noqa: E402
from cpc2_amd.eval import term_discovery as discovery_tool  # noqa: E402
from cpc2_amd.eval.ABX.abx_iterators import normalize_with_singularity  # noqa: E402

D_SAME, D_DIFF, THETA, GAMMA = 0.0, 0.5, 0.25, 0.125


def draw_units(rng, n, n_units):
    """n frames of unit ids in runs of 1 .. 5 frames (vectorised: more runs than needed, cut)."""
    runs = rng.integers(1, 6, n)
    return np.repeat(rng.integers(0, n_units, n), runs)[:n].astype(np.int32)


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / 1e3


def one_hot(units, n_units):
    """The dense tools' frames of these units in cosine mode, on the device: [total, dp] f32."""
    rows = torch.zeros(units.numel(), n_units, dtype=torch.float32, device=units.device)
    rows.scatter_(1, units.long().view(-1, 1), 1.0)
    rows = normalize_with_singularity(rows)
    dp = -(-rows.size(1) // 4) * 4
    if dp == rows.size(1):
        return rows
    frames = torch.zeros(units.numel(), dp, dtype=torch.float32, device=units.device)
    frames[:, :rows.size(1)] = rows
    return frames


def abx_units(units, off, lens_d, lists, n_seg, max_row, max_col, n_pairs):
    lib = _lib.load()
    dev = units.device
    nbytes = lib.cpc_abx_dtw_units_scratch_bytes(n_seg, max_row, max_col)
    scratch = _lib.scratch(nbytes, dev, tag="abx_units_bench") if nbytes else None
    out = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    _lib.check(lib.cpc_abx_dtw_units(_lib.ptr(units), _lib.ptr(off), _lib.ptr(lens_d), int(lens_d.numel()), *[_lib.ptr(x) for x in lists],
                                     n_seg, max_row, max_col, D_SAME, D_DIFF, _lib.ptr(out), None, _lib.ptr(scratch), nbytes,
                                     _lib.stream_ptr(dev)), "cpc_abx_dtw_units")
    return out


def workload(kind, lens, plan, n_units_list, rounds, dense_above, rng, dev):
    """One work list at every alphabet size: the three kernels in alternating rounds."""
    seg_row, seg_start, pair_col = plan[:3]
    rows_of_pairs = np.repeat(seg_row, np.diff(seg_start))
    cells = int((lens[rows_of_pairs] * lens[pair_col]).sum())
    max_row, max_col = int(lens[seg_row].max()), int(lens[pair_col].max())
    lists = [torch.from_numpy(x).to(dev) for x in (seg_row, seg_start, pair_col)]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int32)).to(dev)
    lens_d = torch.from_numpy(lens.astype(np.int32)).to(dev)
    res = {"pairs": int(len(pair_col)), "segments": int(len(seg_row)), "cells": cells, "frames": int(lens.sum()), "max_row": max_row,
           "max_col": max_col}
    for n_units in n_units_list:
        units = torch.from_numpy(np.concatenate([draw_units(rng, int(n), n_units) for n in lens])).to(dev)
        frames = one_hot(units, n_units)

        def run(arm):
            if arm == "abx_units":
                return (abx_units(units, off, lens_d, lists, len(seg_row), max_row, max_col, len(pair_col)),)
            if kind == "sdtw":
                if arm == "units":
                    return td.run_segments_units(units, off, lens_d, *lists, max_row, max_col, D_SAME, D_DIFF)
                return td.run_segments(frames, off, lens_d, *lists, max_row, max_col, td.COSINE)
            if arm == "units":
                return tdisc.run_segments_units(units, off, lens_d, *lists, max_row, max_col, D_SAME, D_DIFF, THETA, GAMMA)
            return tdisc.run_segments(frames, off, lens_d, *lists, max_row, max_col, td.COSINE, THETA, GAMMA)

        arms = ["units", "abx_units", "dense"]
        outs = {arm: run(arm) for arm in arms}                   # warm-up of all
        torch.cuda.synchronize()
        times = {arm: [] for arm in arms}
        for _round in range(rounds if n_units <= dense_above else max(1, rounds - 1)):
            for arm in arms:
                out, s = event_time(lambda: run(arm))
                times[arm].append(s)
                assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out, outs[arm]))   # the same bits
        same = bool(torch.equal(outs["units"][0].view(torch.int32), outs["dense"][0].view(torch.int32)) and
                    torch.equal(outs["units"][1], outs["dense"][1]))
        entry = {"feature_bytes": frames.numel() * 4, "unit_bytes": units.numel() * 4, "feature_columns": int(frames.size(1)),
                 "units_equal_dense_bits": same}
        for arm in arms:
            t = times[arm]
            entry[arm] = {"kernel_s": [round(x, 5) for x in t], "kernel_best_s": min(t), "kernel_spread": (max(t) - min(t)) / min(t),
                          "cells_per_s": cells / min(t)}
        entry["dense_over_units"] = entry["dense"]["kernel_best_s"] / entry["units"]["kernel_best_s"]
        entry["units_over_abx_units"] = entry["units"]["kernel_best_s"] / entry["abx_units"]["kernel_best_s"]
        res[str(n_units)] = entry
        print(f"{kind} {n_units} units: " + ", ".join(f"{arm} {entry[arm]['kernel_best_s']:.4f} s" for arm in arms), file=sys.stderr, flush=True)
        del frames, units, outs
        torch.cuda.empty_cache()
    return res


def hour_files(root, n_files, n_frames, n_units, rng):
    names = [f"utt{k:04d}" for k in range(n_files)]
    utts = [draw_units(rng, n_frames, n_units) for _ in names]
    for k in range(50):                                          # 50 strings of 50 .. 150 frames stand in two files each
        src, dst = k % n_files, (k * 7 + 3) % n_files
        n = int(rng.integers(50, 151))
        o, at = int(rng.integers(0, n_frames - n)), int(rng.integers(0, n_frames - n))
        if dst != src:
            utts[dst][at:at + n] = utts[src][o:o + n]
    path = os.path.join(root, "quantized_outputs.txt")
    with open(path, "w") as f:
        for name, v in zip(names, utts):
            f.write(f"{name}\t" + ",".join(str(u) for u in v) + "\n")
    return path, names, utts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--docs", type=int, default=2000)
    ap.add_argument("--utts", type=int, default=360)
    ap.add_argument("--units", type=int, nargs="+", default=[50, 200, 2000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dense_above", type=int, default=200, help="Alphabets above this run one round fewer (the dense arm is long)")
    ap.add_argument("--hour_docs", type=int, default=450)
    ap.add_argument("--hour_units", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "term_units_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    res = {"workload": {"queries": a.queries, "docs": a.docs, "utterances": a.utts, "units": a.units, "runs": "1..5", "seed": a.seed,
                        "d_same": D_SAME, "d_diff": D_DIFF, "theta": THETA, "gamma": GAMMA, "rounds": a.rounds}}

    # ---- term detection: the work list of term_detection_bench.py ----
    doc_lens = rng.integers(300, 1501, a.docs)
    q_lens = rng.integers(50, 151, a.queries)
    lens = np.concatenate([doc_lens, q_lens]).astype(np.int64)
    plan = td.plan_segments(np.arange(a.docs, a.docs + a.queries), np.arange(a.docs), lens)
    res["detection"] = workload("sdtw", lens, plan, a.units, a.rounds, a.dense_above, rng, dev)

    # ---- term discovery: the work list of term_discovery_bench.py ----
    lens = rng.integers(300, 1501, a.utts).astype(np.int64)
    plan = tdisc.plan_pairs(np.arange(a.utts), lens)
    res["discovery"] = workload("align", lens, plan, a.units, a.rounds, a.dense_above, rng, dev)

    # ---- the tools on a synthetic hour of units ----
    with tempfile.TemporaryDirectory(prefix="term_units_bench_") as tmp:
        os.makedirs(os.path.join(tmp, "det"))
        path, names, utts = hour_files(os.path.join(tmp, "det"), a.hour_docs, 800, a.hour_units, rng)
        with open(os.path.join(tmp, "q.txt"), "w") as q, open(os.path.join(tmp, "r.txt"), "w") as r:
            for k in range(50):
                q.write(f"q{k} {names[k % a.hour_docs]} {1.0 + 0.002:.3f} {2.0 + 0.008:.3f}\n")
                r.write(f"q{k} {names[(k * 7 + 3) % a.hour_docs]}\n")
        t0 = time.perf_counter()
        out = detection_tool.main(["from_units", path, "--queries", os.path.join(tmp, "q.txt"), "--relevance", os.path.join(tmp, "r.txt"),
                                   "--out", os.path.join(tmp, "det_out")])
        log = json.load(open(os.path.join(tmp, "det_out", "term_detection_log.json")))
        res["detection_tool_synthetic_hour"] = {"wall_s": time.perf_counter() - t0, "map": out["scores"]["map"], **log}
        os.makedirs(os.path.join(tmp, "disc"))
        path, names, utts = hour_files(os.path.join(tmp, "disc"), a.utts, 1000, a.hour_units, rng)
        t0 = time.perf_counter()
        out = discovery_tool.main(["from_units", path, "--threshold", str(THETA), "--gap_penalty", str(GAMMA), "--out",
                                   os.path.join(tmp, "disc_out")])
        log = {k: v for k, v in out["log"].items() if k != "args"}
        res["discovery_tool_synthetic_hour"] = {"wall_s": time.perf_counter() - t0, **log}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
