#!/usr/bin/env python3
"""Timings of the `pitch_wsola` pitch shift on one MI355X.  Prints one JSON object and writes it to --out.

  1. cpc_augment_pitch (csrc/pitch.hip: the search kernel, then the synthesis kernel) at b = 8 and 64, W = 20480, cents = +-300
     alternating over the rows, by device events.  The entry launches both kernels, so the two are told apart by a second arm: the
     same batch and the same table of segments with every cents == 0, where the search does all its work and the synthesis is a
     copy.  `search_us` is that arm less the copy's bytes at the HBM rate, `synthesis_us` is the full entry less `search_us`.
     The arms ALTERNATE, round by round; a figure is the median over the rounds with the smallest and largest beside it.  Beside
     them the floor -- the bytes the shift has to move (a window read, a window written) at the HBM rate -- and the float64 numpy
     statement of tests/pitch_oracle.py on the host (time per window, and the largest difference).
  2. cpc2_amd.train.trainStep on the window feeder at CPC-small, b = 64, with the past half augmented by --augment_type none /
     pitch_wsola / pitch_wsola time_dropout, arms alternating epoch by epoch as tools/augment_bench.py does.

    python tools/pitch_bench.py [--quick] [--out profiles/pitch_bench.json]"""
import argparse
import contextlib
import copy
import io
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cpc2_amd import _lib  # noqa: E402
from cpc2_amd import data_augmentation as da  # noqa: E402
from cpc2_amd._lib import stream_ptr  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak (tools/augment_bench.py)
W = 20480


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def spread(values):
    s = sorted(values)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def kernel_case(b, warmup, iters, rounds, host_rows):
    import pitch_oracle as PO
    g = torch.Generator().manual_seed(b)
    t = torch.arange(W, dtype=torch.float32)
    x = (torch.randn(b, W, generator=g) * 0.1 * (0.3 + torch.sin(t / 700.0) ** 2)).contiguous()
    xd = x.to(DEV)
    cents = [300 if i % 2 == 0 else -300 for i in range(b)]
    full = da.pitch_tables(cents, W)
    J = full["nominal"].shape[1]
    still = da.pitch_tables([0] * b, W, segments=J)
    still["nominal"] = full["nominal"]                   # the search walks the same candidates; only the synthesis becomes a copy
    dev = {name: {k: torch.from_numpy(tab[k]).to(DEV) for k in ("cents", "ratio", "cutoff", "nominal")}
           for name, tab in (("full", full), ("still", still))}
    out = torch.empty(b, W, device=DEV)

    def run(name):
        return da._pitch_launch(xd, dev[name], 0, b, 300, W, out)

    times = {"full": [], "still": []}
    for _ in range(rounds):
        for name in times:                               # alternating arms
            times[name].append(timed(lambda: run(name), warmup, iters))
    q = run("full")
    torch.cuda.synchronize()
    y = out.double().cpu().numpy()
    t0 = time.perf_counter()
    want, want_q, bound = PO.pitch_batch(x[:host_rows].numpy(), cents[:host_rows], J)
    host_s = (time.perf_counter() - t0) / host_rows
    err = np.abs(y[:host_rows] - want)
    nbytes = 2 * 4 * b * W
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    entry, arm = spread(times["full"]), spread(times["still"])
    search_us = arm["median"] - floor_us
    return dict(b=b, W=W, cents="+300 / -300 alternating", segments=J, entry_us=entry, search_and_copy_us=arm,
                search_us=search_us, synthesis_us=entry["median"] - search_us, bytes=nbytes, floor_us=floor_us,
                entry_over_floor=entry["median"] / floor_us, rounds=rounds, iters=iters,
                host_statement_ms_per_window=host_s * 1e3, host_over_device=host_s * 1e6 * b / entry["median"],
                starts_equal_host=bool(np.array_equal(q.cpu().numpy()[:host_rows], want_q)),
                max_abs_diff_vs_host=float(err.max()), worst_error_over_bound=float((err / np.maximum(bound, 1e-300)).max()))


def feeder_arms(batch, steps, rounds, quick):
    import bench
    from cpc2_amd.dataset import AudioBatchData, findAllSeqs
    from cpc2_amd.train import DataParallelContext, trainStep
    cfg = bench.CONFIGS["small_feeder"]
    tmp = tempfile.mkdtemp(prefix="cpc_pitch_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        bench.write_synthetic_corpus(os.path.join(tmp, "speech"), steps * batch, seed=7)
        random.seed(11)
        np.random.seed(11)
        seqs, speakers = findAllSeqs(os.path.join(tmp, "speech"), extension=".wav")
        arms = {"none": None, "pitch_wsola": da.PitchShiftAugment(300),
                "pitch_wsola+time_dropout": da.CombinedTransforms(["pitch_wsola", "time_dropout"], shift_max=300, t_ms=100)}
        if quick:
            arms = {k: arms[k] for k in ("none", "pitch_wsola")}
        with contextlib.redirect_stdout(io.StringIO()):
            base = AudioBatchData(os.path.join(tmp, "speech"), W, seqs, None, len(speakers), device=DEV)
        data = {}
        for name, aug in arms.items():                              # one pack, resident once: the arms differ in the augmentation only
            data[name] = copy.copy(base)
            data[name].augment_past, data[name].augmentation = aug is not None, aug
        model, crit, opt = bench.build(cfg, DEV)
        dp = DataParallelContext(opt, early_params=list(crit.parameters()) + list(model.gAR.parameters()), timing=False)
        crit.seed(1234)
        crit.sampler.prefetch = True
        times = {name: [] for name in arms}

        def epoch(name):
            loader = data[name].getDataLoader(batch, "samespeaker", True)
            with contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                logs = trainStep(loader, model, crit, opt, None, 1000, dp=dp)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / max(1, int(logs["iter"]))

        for name in arms:                                           # warm-up: whole epochs, every arm
            for _ in range(1 if quick else 2):
                epoch(name)
        for _ in range(rounds):
            for name in arms:                                       # alternating arms
                times[name].append(epoch(name))
        plan_us = {}
        for name in arms:                                           # the host side alone: a pack's sampler draws and its plan
            loader = data[name].getDataLoader(batch, "samespeaker", True)
            t0 = time.perf_counter()
            batches, _plans = loader.pack_plan()
            torch.cuda.synchronize()
            plan_us[name] = 1e6 * (time.perf_counter() - t0) / max(1, len(batches))
        _lib.check(_lib.load().cpc_async_error_check(stream_ptr(DEV)), "async error check")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for name, ts in times.items():
        s = spread(ts)
        out[name] = dict(ms_per_step_median=s["median"], ms_per_step_min=s["min"], ms_per_step_max=s["max"], rounds=len(ts),
                         host_plan_us_per_step=plan_us[name])
    for name in out:
        out[name]["over_none_ms"] = out[name]["ms_per_step_median"] - out["none"]["ms_per_step_median"]
    return dict(config="CPC-small (hidden 256, GRU, 12 predictions, 128 negatives)", batch=batch, steps_per_epoch=steps, arms=out,
                note="host clock around one epoch of trainStep ending in a device synchronise; the plan of the pack is drawn inside "
                     "the timed epoch, before its first step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one size, few repetitions")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--kernel_rounds", type=int, default=5, help="alternating rounds of the two kernel arms")
    ap.add_argument("--steps", type=int, default=100, help="steps per feeder epoch")
    ap.add_argument("--rounds", type=int, default=5, help="timed epochs per feeder arm")
    ap.add_argument("--no_feeder", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pitch_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if args.quick:
        res["kernels"] = [kernel_case(8, 2, 5, 2, 2)]
        if not args.no_feeder:
            res["feeder"] = feeder_arms(64, 30, 1, True)
    else:
        res["kernels"] = [kernel_case(b, args.warmup, args.iters, args.kernel_rounds, 4) for b in (8, 64)]
        if not args.no_feeder:
            res["feeder"] = feeder_arms(64, args.steps, args.rounds, False)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
