#!/usr/bin/env python3
"""Timings of the `freeverb` reverberation on one MI355X.  Prints one JSON object and writes it to --out.

  1. cpc_augment_freeverb (csrc/freeverb.hip) at b = 64, W = 20480 by device events, for room sizes all 0, all 50, all 99 and
     drawn (np.random.randint(0, 100) per window), beside cpc_augment_fir -- natural_reverb's kernel, the alternative a user with
     a corpus of impulse responses has -- on the same batch with one 0.5 s response (8000 taps) per window.  The arms ALTERNATE,
     round by round; a figure is the median over the rounds with the smallest and largest beside it.  Beside them the floor: the
     bytes the effect has to move (a window read, a window written) at the HBM rate.  No time is fixed in advance; the FIR may win.
  2. The numpy statement of tests/freeverb_oracle.py on the host: seconds per window in float64, the largest difference of the
     kernel from it, the float32 statement's own error E32, their ratio (the accuracy tests' yardstick), and whether the kernel
     equals the float32 statement.
  3. cpc2_amd.train.trainStep on the window feeder at CPC-small, b = 64, with the past half augmented by --augment_type none /
     freeverb / freeverb time_dropout, arms alternating epoch by epoch as tools/augment_bench.py does.

    python tools/freeverb_bench.py [--quick] [--out profiles/freeverb_bench.json]"""
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
from cpc2_amd._lib import check, ptr, stream_ptr  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak (tools/augment_bench.py)
W = 20480
FIR_TAPS = 8000                   # 0.5 s at 16 kHz


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
    import freeverb_oracle as FO
    lib = _lib.load()
    g = torch.Generator().manual_seed(b)
    x = (torch.randn(b, W, generator=g) * 0.05).contiguous()
    xd = x.to(DEV)
    np.random.seed(5)
    drawn = [int(np.random.randint(0, 100)) for _ in range(b)]
    rooms = {"rs=0": [0] * b, "rs=50": [50] * b, "rs=99": [99] * b, "drawn": drawn}
    tables = {name: da.freeverb_tables(r) for name, r in rooms.items()}
    comb = {name: torch.from_numpy(t["comb_len"]).to(DEV) for name, t in tables.items()}
    out = torch.empty(b, W, device=DEV)

    # the FIR arm: one 0.5 s response per window, an exponentially decaying noise
    decay = torch.exp(-torch.arange(FIR_TAPS, dtype=torch.float32) / 1500.0)
    ir = (torch.randn(b, FIR_TAPS, generator=g) * decay).contiguous().view(-1).to(DEV)
    ir_off = (torch.arange(b, dtype=torch.int64) * FIR_TAPS).to(DEV)
    ir_len = torch.full((b,), FIR_TAPS, dtype=torch.int32, device=DEV)
    scratch = _lib.scratch(lib.cpc_augment_fir_scratch_bytes(b, W), DEV, tag="augment_fir")

    def freeverb(name):
        return da._freeverb_launch(xd, comb[name], 0, b, tables[name], W, out)

    def fir():
        check(lib.cpc_augment_fir(ptr(xd), ptr(ir), ir.numel(), ptr(ir_off), ptr(ir_len), ptr(out), ptr(scratch), scratch.numel(), b, W,
                                  stream_ptr(DEV)), "augment_fir")

    arms = {name: (lambda name=name: freeverb(name)) for name in rooms}
    arms["fir_0.5s"] = fir
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():                    # alternating arms
            times[name].append(timed(fn, warmup, iters))
    nbytes = 2 * 4 * b * W
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    res = dict(b=b, W=W, bytes=nbytes, floor_us=floor_us, rounds=rounds, iters=iters, fir_taps=FIR_TAPS,
               us={name: spread(ts) for name, ts in times.items()})
    res["drawn_over_floor"] = res["us"]["drawn"]["median"] / floor_us
    res["drawn_over_fir"] = res["us"]["drawn"]["median"] / res["us"]["fir_0.5s"]["median"]

    # the statement on the host, on the first rows of the drawn arm
    freeverb("drawn")
    torch.cuda.synchronize()
    got = out[:host_rows].cpu().numpy()
    t0 = time.perf_counter()
    y64 = FO.freeverb(x[:host_rows].numpy(), drawn[:host_rows], dtype=np.float64)
    host_s = (time.perf_counter() - t0) / host_rows
    y32 = FO.freeverb(x[:host_rows].numpy(), drawn[:host_rows], dtype=np.float32)
    e32 = float(np.abs(y32.astype(np.float64) - y64).max())
    err = float(np.abs(got.astype(np.float64) - y64).max())
    yard = max(e32, 2.0 ** -24 * float(np.abs(y64).max()))
    res["host"] = dict(rows=host_rows, statement_f64_ms_per_window=host_s * 1e3,
                       host_over_device=host_s * 1e6 * b / res["us"]["drawn"]["median"], max_abs_diff_vs_f64=err, E32=e32,
                       yardstick=yard, error_over_yardstick=err / yard, equals_f32_statement=bool(np.array_equal(got, y32)))
    return res


def feeder_arms(batch, steps, rounds, quick, arms=None):
    """`arms`: {name: transform or None} with a "none" arm, for another augmentation's tool (tools/bandreject_bench.py)."""
    import bench
    from cpc2_amd.dataset import AudioBatchData, findAllSeqs
    from cpc2_amd.train import DataParallelContext, trainStep
    cfg = bench.CONFIGS["small_feeder"]
    tmp = tempfile.mkdtemp(prefix="cpc_freeverb_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        bench.write_synthetic_corpus(os.path.join(tmp, "speech"), steps * batch, seed=7)
        random.seed(11)
        np.random.seed(11)
        seqs, speakers = findAllSeqs(os.path.join(tmp, "speech"), extension=".wav")
        if arms is None:
            arms = {"none": None, "freeverb": da.FreeverbAugment(),
                    "freeverb+time_dropout": da.CombinedTransforms(["freeverb", "time_dropout"], t_ms=100)}
            if quick:
                arms = {k: arms[k] for k in ("none", "freeverb")}
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
        _lib.check(_lib.load().cpc_async_error_check(stream_ptr(DEV)), "async error check")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for name, ts in times.items():
        s = spread(ts)
        out[name] = dict(ms_per_step_median=s["median"], ms_per_step_min=s["min"], ms_per_step_max=s["max"], rounds=len(ts))
    for name in out:
        out[name]["over_none_ms"] = out[name]["ms_per_step_median"] - out["none"]["ms_per_step_median"]
    return dict(config="CPC-small (hidden 256, GRU, 12 predictions, 128 negatives)", batch=batch, steps_per_epoch=steps, arms=out,
                note="host clock around one epoch of trainStep ending in a device synchronise; the plan of the pack is drawn inside "
                     "the timed epoch, before its first step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="few repetitions")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--kernel_rounds", type=int, default=5, help="alternating rounds of the kernel arms")
    ap.add_argument("--steps", type=int, default=100, help="steps per feeder epoch")
    ap.add_argument("--rounds", type=int, default=5, help="timed epochs per feeder arm")
    ap.add_argument("--no_feeder", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("freeverb_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if args.quick:
        res["kernels"] = [kernel_case(64, 2, 5, 2, 1)]
        if not args.no_feeder:
            res["feeder"] = feeder_arms(64, 30, 1, True)
    else:
        res["kernels"] = [kernel_case(64, args.warmup, args.iters, args.kernel_rounds, 4)]
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
