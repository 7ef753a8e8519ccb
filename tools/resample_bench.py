#!/usr/bin/env python3
"""Timings of the sample-rate conversion on one MI355X.  Prints one JSON object and writes it to --out.

  1. cpc_resample at 48 -> 16, 32 -> 16, 44.1 -> 16 and 8 -> 16 kHz, on one 60 s signal and on a pack of 2 000 one-second
     signals (an impulse-response directory), beside
       - the same table applied by torch.nn.functional.conv1d(stride=o) on the device, with the [frames][phases] transposition
         that gives the samples their order -- the formulation torchaudio uses,
       - the floor out_samples x taps multiply-adds at the 78.6 TFLOP/s of an unpacked v_fma_f32 stream,
       - the floor (in + out) bytes at the HBM rate.
     The two arms ALTERNATE, round by round, inside this one process; a figure is the median over the rounds.
  2. the PCM16 quantiser on the 60 s outputs.
  3. cpc2_amd.eval.utils.adjust_sample_rate on a synthetic directory of 44.1 kHz PCM16 .wav files, its wall time split into
     decode, upload, kernel, quantise (with the download) and write.

    python tools/resample_bench.py [--quick] [--out profiles/resample_bench.json]
Kernel times are device events around --iters repetitions after --warmup ones."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd import _lib, audio  # noqa: E402
from cpc2_amd._lib import check, ptr, stream_ptr  # noqa: E402
from cpc2_amd.eval.utils import adjust_sample_rate as asr  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak
F32_FLOPS = 78.6e12               # unpacked v_fma_f32 (this library builds without packed f32)
RATES = [(48000, 16000), (32000, 16000), (44100, 16000), (8000, 16000)]


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
    return a.elapsed_time(b) / iters


def median(values):
    s = sorted(values)
    return s[len(s) // 2]


def kernel_case(orig, new, count, seconds, warmup, iters, rounds):
    o, n, w, taps = audio.resample_plan(orig, new)
    length = int(orig * seconds)
    out_len = audio.output_length(length, o, n)
    frames = -(-out_len // n)
    g = torch.Generator(device=DEV).manual_seed(orig + count)
    x = torch.randn(count, length, device=DEV, generator=g) * 0.1
    table = audio.resample_table(orig, new).to(DEV)
    tables = torch.tensor([[r * length for r in range(count)], [length] * count, [r * out_len for r in range(count)]],
                          dtype=torch.int64).to(DEV)
    y = torch.empty(count, out_len, device=DEV)
    lib, st = _lib.load(), stream_ptr(DEV)
    weight = table.view(n, 1, taps)
    pad_right = (frames - 1) * o + taps - (w + length)

    def ours():
        check(lib.cpc_resample(ptr(x), x.numel(), ptr(tables[0]), ptr(tables[1]), count, length, ptr(table), o, n, w, ptr(y),
                               y.numel(), ptr(tables[2]), st), "resample")

    def conv_only():
        xp = torch.nn.functional.pad(x, (w, pad_right)).unsqueeze(1)
        return torch.nn.functional.conv1d(xp, weight, stride=o)                         # [count, n, frames]

    def conv():
        return conv_only().transpose(1, 2).reshape(count, -1)[:, :out_len].contiguous()

    ours()
    conv_error = None
    try:
        err = float((y - conv()).abs().max())
    except RuntimeError as e:                                                           # (the convolution library refused the shape)
        conv_error, err = str(e).splitlines()[0][:200], float("nan")
    t_ours, t_conv, t_conv_only = [], [], []
    for _ in range(rounds):                                                             # alternating arms
        t_ours.append(timed(ours, warmup, iters))
        t_conv.append(timed(conv, warmup, iters) if conv_error is None else float("nan"))
        t_conv_only.append(timed(conv_only, warmup, iters) if conv_error is None else float("nan"))
    macs = count * out_len * taps
    nbytes = 4 * count * (length + out_len)
    ours_us = median(t_ours) * 1e3
    fma_floor_us, hbm_floor_us = 2 * macs / F32_FLOPS * 1e6, nbytes / HBM_BYTES_PER_S * 1e6
    res = dict(orig=orig, new=new, o=o, n=n, taps=taps, signals=count, seconds=seconds, out_samples=count * out_len,
               ours_us=ours_us, ours_us_min=min(t_ours) * 1e3, ours_us_max=max(t_ours) * 1e3,
               conv1d_us=median(t_conv) * 1e3, conv1d_without_transpose_us=median(t_conv_only) * 1e3,
               speedup_vs_conv1d=median(t_conv) / median(t_ours), multiply_adds=macs,
               achieved_tflops=2 * macs / (ours_us * 1e-6) / 1e12, fma_floor_us=fma_floor_us, hbm_floor_us=hbm_floor_us,
               bound="FMA" if fma_floor_us > hbm_floor_us else "HBM bytes",
               share_of_floor=max(fma_floor_us, hbm_floor_us) / ours_us, max_abs_diff_vs_conv1d=err, rounds=rounds)
    if conv_error is not None:
        res["conv1d_error"] = conv_error
    if count == 1:
        clamped = torch.zeros(1, dtype=torch.int64, device=DEV)
        q = torch.empty(y.shape, dtype=torch.int16, device=DEV)
        t_q = timed(lambda: check(lib.cpc_resample_to_pcm16(ptr(y), y.numel(), ptr(q), ptr(clamped), st), "pcm16"), warmup, iters)
        res["pcm16_us"] = t_q * 1e3
    return res


def tool_case(files, seconds, rate, target, rounds):
    tmp = tempfile.mkdtemp(prefix="cpc_resample_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        rng = np.random.RandomState(5)
        src = os.path.join(tmp, "src")
        os.makedirs(src)
        for i in range(files):
            samples = (rng.randn(1, int(rate * seconds)) * 3000).astype(np.int16)
            audio.write_wav(os.path.join(src, f"file_{i:05d}.wav"), samples, rate)
        names = sorted(os.listdir(src))
        runs = []
        for r in range(rounds + 1):                                    # (the first run warms the table, the allocator, the page cache)
            out = os.path.join(tmp, f"out_{r}")
            os.makedirs(out)
            timings = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            asr.adjust_sample_rate(src, names, out, target, timings=timings)
            torch.cuda.synchronize()
            timings["wall"] = time.perf_counter() - t0
            if r:
                runs.append(timings)
            shutil.rmtree(out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = {k + "_s": median([t.get(k, 0.0) for t in runs]) for k in ("wall", "decode", "upload", "kernel", "quantise", "write")}
    res.update(files=files, seconds_each=seconds, rate=rate, target=target, audio_seconds=files * seconds, rounds=rounds,
               audio_seconds_per_wall_second=files * seconds / res["wall_s"],
               note="PCM16 .wav in a memory-backed directory when there is one; the device is synchronised between the stages; "
                    "quantise includes the download of the int16 samples")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no_tool", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if args.quick:
        res["kernel"] = [kernel_case(44100, 16000, 1, 10.0, 1, 3, 1), kernel_case(48000, 16000, 50, 1.0, 1, 3, 1)]
        if not args.no_tool:
            res["tool"] = tool_case(8, 2.0, 44100, 16000, 1)
    else:
        res["kernel"] = [kernel_case(a, b, c, s, args.warmup, args.iters, args.rounds) for a, b in RATES for c, s in ((1, 60.0), (2000, 1.0))]
        if not args.no_tool:
            res["tool"] = tool_case(360, 10.0, 44100, 16000, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
