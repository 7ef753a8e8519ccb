#!/usr/bin/env python3
"""Timings of the `bandreject_sinc` filter on one MI355X.  Prints one JSON object and writes it to --out.

  1. cpc_augment_bandreject (csrc/bandreject.hip) at b = 64 and 128 windows of W = 20480 samples, for half lengths 157 (the
     default design) and 1024 (the longest), bands drawn as the transform draws them, by device events.  Beside it, on the same rows:
       * cpc_augment_fir -- natural_reverb's kernel, the closest existing one: causal, float32, peak-normalised -- with the same
         2 H + 1 taps rounded to float32 as every window's response;
       * torch.nn.functional.conv1d with one filter per row (groups = b) in float32 and in float64 (an arm that torch refuses is
         recorded as its error);
       * cpc_bandreject_taps alone: what designing the taps once per row costs (the filter kernel designs them once per TILE).
     The arms ALTERNATE, round by round; a figure is the median over the rounds with the smallest and largest beside it.
     The floors: the bytes the filter has to move (a window read, a window written) at the HBM rate, and its float64 operations
     (H + 1 FMAs and H additions per output) at the float64 vector rate -- taken as one v_fma_f64 per lane per clock, half the
     FP32 vector peak of 157.3 TFLOPS, since the packed float32 forms have no float64 counterpart.  No time is fixed in advance.
  2. cpc2_amd.train.trainStep on the window feeder at CPC-small, b = 64, with the past half augmented by --augment_type none /
     bandreject_sinc / bandreject_sinc time_dropout, arms alternating epoch by epoch (tools/freeverb_bench.py's feeder_arms).

    python tools/bandreject_bench.py [--quick] [--out profiles/bandreject_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cpc2_amd import _lib  # noqa: E402
from cpc2_amd import data_augmentation as da  # noqa: E402
from cpc2_amd._lib import check, ptr, stream_ptr  # noqa: E402
from freeverb_bench import DEV, HBM_BYTES_PER_S, W, feeder_arms, spread, timed  # noqa: E402

F64_FMA_PER_S = 157.3e12 / 4      # 78.6 TFLOPS of float64 vector work, two operations per FMA
DESIGNS = {157: (120.0, 400.0), 1024: (120.0, 61.0)}      # half length: (attenuation in dB, transition width in Hz)


def kernel_case(b, half, warmup, iters, rounds):
    import bandreject_oracle as BO
    lib = _lib.load()
    g = torch.Generator().manual_seed(b + half)
    x = (torch.randn(b, W, generator=g) * 0.05).contiguous()
    xd = x.to(DEV)
    np.random.seed(5)
    aug = da.BandrejectSincAugment(1.0, *DESIGNS[half])
    plan = aug.seal([aug.draw_one(W) for _ in range(b)], DEV)
    assert plan["half"] == half
    band = plan["_dev"]["band"]
    out = torch.empty(b, W, device=DEV)
    taps_out = torch.empty(b, half + 1, dtype=torch.float64, device=DEV)

    # the comparators' taps: the statement's, [b, 2 H + 1]
    h64 = np.stack([BO.taps(lo, hi, half, plan["beta"]) for lo, hi in plan["band"]])
    h32 = torch.from_numpy(h64.astype(np.float32)).to(DEV)
    count = 2 * half + 1
    ir = h32.contiguous().view(-1)
    ir_off = (torch.arange(b, dtype=torch.int64) * count).to(DEV)
    ir_len = torch.full((b,), count, dtype=torch.int32, device=DEV)
    scratch = _lib.scratch(lib.cpc_augment_fir_scratch_bytes(b, W), DEV, tag="augment_fir")
    w32, w64 = h32.view(b, 1, count), torch.from_numpy(h64).to(DEV).view(b, 1, count)
    x64 = xd.double()

    def bandreject():
        return da._bandreject_launch(xd, band, 0, b, plan, W, out)

    def design():
        check(lib.cpc_bandreject_taps(ptr(band), b, half, plan["beta"], float(da.BANDREJECT_SR), ptr(taps_out), stream_ptr(DEV)),
              "bandreject_taps")

    def fir():
        check(lib.cpc_augment_fir(ptr(xd), ptr(ir), ir.numel(), ptr(ir_off), ptr(ir_len), ptr(out), ptr(scratch), scratch.numel(), b, W,
                                  stream_ptr(DEV)), "augment_fir")

    arms = {"bandreject": bandreject, "taps_only": design, "fir_f32": fir,
            "conv1d_f32": lambda: torch.nn.functional.conv1d(xd.view(1, b, W), w32, padding=half, groups=b),
            "conv1d_f64": lambda: torch.nn.functional.conv1d(x64.view(1, b, W), w64, padding=half, groups=b)}
    refused = {}
    for name in ("conv1d_f32", "conv1d_f64"):
        try:
            arms[name]()
            torch.cuda.synchronize()
        except RuntimeError as err:
            refused[name] = str(err).splitlines()[0][:200]
            del arms[name]
    # an arm that takes more than 20 ms a call (a convolution torch has no fast path for) is repeated twice a round, not `iters` times
    slow = {name for name, fn in arms.items() if timed(fn, 1, 1) > 20e3}
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():                    # alternating arms
            times[name].append(timed(fn, 0, 2) if name in slow else timed(fn, warmup, iters))
    nbytes = 2 * 4 * b * W
    fmas = b * W * (half + 1)
    res = dict(b=b, W=W, half=half, taps=count, attenuation_dB=DESIGNS[half][0], transition_hz=DESIGNS[half][1], rounds=rounds,
               iters=iters, bytes=nbytes, bytes_floor_us=nbytes / HBM_BYTES_PER_S * 1e6, f64_fmas=fmas, f64_adds=b * W * half,
               f64_floor_us=(fmas + b * W * half) / F64_FMA_PER_S * 1e6, us={name: spread(ts) for name, ts in times.items()},
               refused=refused, two_calls_per_round=sorted(slow))
    mine = res["us"]["bandreject"]["median"]
    res["over_f64_floor"] = mine / res["f64_floor_us"]
    res["over_bytes_floor"] = mine / res["bytes_floor_us"]
    for name in arms:
        if name != "bandreject":
            res["over_" + name] = mine / res["us"][name]["median"]
    # what the kernel computes against the statement, on the first rows
    bandreject()
    torch.cuda.synchronize()
    rows = 2
    want = BO.bandreject(x[:rows].numpy(), plan["low"][:rows], plan["high"][:rows], half, plan["beta"])
    err = np.abs(out[:rows].cpu().numpy().astype(np.float64) - want)
    bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -38 * BO.reach(x[:rows].numpy(), half) + 2.0 ** -149
    res["host"] = dict(rows=rows, max_abs_diff_vs_f64=float(err.max()), error_over_bound=float((err / bound).max()))
    return res


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
        raise SystemExit("bandreject_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tile": _lib.load().cpc_bandreject_tile()}
    warmup, iters, rounds = (2, 5, 2) if args.quick else (args.warmup, args.iters, args.kernel_rounds)
    res["kernels"] = [kernel_case(b, half, warmup, iters, rounds) for half in DESIGNS for b in (64, 128)]
    if not args.no_feeder:
        arms = {"none": None, "bandreject_sinc": da.BandrejectSincAugment()}
        if not args.quick:
            arms["bandreject_sinc+time_dropout"] = da.CombinedTransforms(["bandreject_sinc", "time_dropout"], t_ms=100,
                                                                         bandreject_scaler=1.0)
        res["feeder"] = feeder_arms(64, 30 if args.quick else args.steps, 1 if args.quick else args.rounds, args.quick, arms)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
