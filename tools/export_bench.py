#!/usr/bin/env python3
"""Timings of the feature export on one MI355X.  Prints one JSON object and writes it to --out.

  1. cpc2_amd.text.format_rows on a [100 000, 256] matrix of N(0, 0.3^2) values (1 000 s of audio at 256 dimensions) with the
     tool's time column as prefixes, beside the reference's loop on the host
         [str(x) for x in [t] + feature[step, :].tolist()]   ->   ' '.join(...) + '\\n'
     in this same process.  The host loop is linear in the rows and slow, so it runs on the first --host_rows rows (its bytes must
     equal the device's for those rows) and its time is scaled to the whole matrix; both arms are repeated --rounds times,
     alternating, and the minimum, median and maximum are given.  The device arm is also split into its parts (the value kernel,
     the row sums, the scan, the pack kernel) by device events around 50 repetitions each, and the copy to pinned memory and
     the write to a file are timed apart.
  2. cpc2_amd.eval.build_zeroSpeech_features on a synthetic hour of audio (360 PCM16 .wav files of 10 s at 16 kHz, a CPC-small
     checkpoint with random weights), wall time by stage, for --format fea and npy.

    python tools/export_bench.py [--quick] [--out profiles/export_bench.json]"""
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
from cpc2_amd import _lib, audio, text  # noqa: E402
from cpc2_amd._lib import check, ptr, stream_ptr  # noqa: E402
from cpc2_amd.eval import build_zeroSpeech_features as bz  # noqa: E402

DEV = torch.device("cuda:0")


def stats(values):
    s = sorted(values)
    return dict(min=s[0], median=s[len(s) // 2], max=s[-1], n=len(s))


def reference_loop(feature, times):
    """The reference's fea lines of a host tensor [frames, dim] (build_zeroSpeech_features.py:70-77), as bytes."""
    out = []
    for step in range(feature.size(0)):
        line = [times[step]] + feature[step, :].tolist()
        line = [str(x) for x in line]
        out.append(' '.join(line) + '\n')
    return "".join(out).encode()


def device_parts(x, prefix, iters):
    """Device-event times of the parts of format_rows, through the library's entry points."""
    lib, st = _lib.load(), stream_ptr(DEV)
    rows, cols = x.shape
    prefix_data, prefix_off = text._prefix_tables(prefix, rows, DEV)
    slots = torch.empty(rows * cols * 3, dtype=torch.int64, device=DEV)
    lens = torch.empty(rows * cols, dtype=torch.uint8, device=DEV)
    row_bytes = torch.empty(rows, dtype=torch.int64, device=DEV)
    state = {}

    def values():
        check(lib.cpc_text_format_f32(ptr(x), rows * cols, ptr(slots), ptr(lens), st), "text_format")

    def sums():
        check(lib.cpc_text_row_bytes(ptr(lens), rows, cols, ptr(prefix_off), ptr(row_bytes), st), "text_row_bytes")

    def scan():
        end = torch.cumsum(row_bytes, 0)
        state["off"], state["end"] = end - row_bytes, end

    def pack():
        check(lib.cpc_text_pack(ptr(slots), ptr(lens), rows, cols, ptr(prefix_data), ptr(prefix_off), ptr(state["off"]), ptr(state["out"]),
                                state["out"].numel(), st), "text_pack")

    res = {}
    for name, fn in (("value_kernel", values), ("row_bytes_kernel", sums), ("scan", scan)):
        fn()
        res[name + "_ms"] = timed(fn, iters)
    state["out"] = torch.empty(int(state["end"][-1]), dtype=torch.uint8, device=DEV)
    pack()
    res["pack_kernel_ms"] = timed(pack, iters)
    res["values_per_second"] = rows * cols / (res["value_kernel_ms"] * 1e-3)
    res["text_bytes"] = state["out"].numel()
    return res


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def format_case(rows, cols, host_rows, rounds, tmp):
    g = torch.Generator().manual_seed(13)
    host = torch.randn(rows, cols, generator=g) * 0.3
    x = host.to(DEV)
    times = bz.frame_times(rows, 0.01)
    host_rows = min(host_rows, rows)
    device_s, host_s, prefix_s, copy_s, write_s = [], [], [], [], []
    buf = text.format_rows(x, [str(t) for t in times])                 # (warm: the allocator, the kernels' code objects)
    want = reference_loop(host[:host_rows], times)
    assert buf[:len(want)].cpu().numpy().tobytes() == want, "the device's text differs from the reference loop's"
    path = os.path.join(tmp, "format_case.fea")
    for _ in range(rounds):                                            # alternating arms
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prefix = [str(t) for t in times]
        t1 = time.perf_counter()
        buf = text.format_rows(x, prefix)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        prefix_s.append(t1 - t0)
        device_s.append(t2 - t1)
        timings = {}
        with open(path, "wb") as f:
            text.write_rows(f, buf, timings)
        copy_s.append(timings["copy"])
        write_s.append(timings["write"])
        t0 = time.perf_counter()
        reference_loop(host[:host_rows], times)
        host_s.append((time.perf_counter() - t0) * rows / host_rows)
    os.remove(path)
    res = dict(rows=rows, cols=cols, audio_seconds=rows * 0.01, text_bytes=buf.numel(), rounds=rounds, host_rows_measured=host_rows,
               device_format_rows_s=stats(device_s), host_time_column_s=stats(prefix_s), copy_to_pinned_s=stats(copy_s),
               write_file_s=stats(write_s), host_reference_loop_s_scaled=stats(host_s),
               note="host_reference_loop_s_scaled: measured on host_rows_measured rows, times rows / host_rows_measured; the file "
                    "is written to a memory-backed directory when there is one")
    res["speedup_format_only"] = res["host_reference_loop_s_scaled"]["median"] / res["device_format_rows_s"]["median"]
    whole = res["device_format_rows_s"]["median"] + res["host_time_column_s"]["median"] + res["copy_to_pinned_s"]["median"]
    res["speedup_with_time_column_and_copy"] = res["host_reference_loop_s_scaled"]["median"] / whole
    res["parts"] = device_parts(x, [str(t) for t in times], 50 if rows >= 100000 else 3)
    return res


def make_checkpoint(run_dir):
    """A CPC-small run directory (the default configuration: 256-dimensional encoder and GRU) with random weights."""
    from cpc2_amd.cpc_default_config import get_default_cpc_config
    from cpc2_amd.feature_loader import save_checkpoint
    from cpc2_amd.model import CPCModel
    from cpc2_amd.train import getAR, getEncoder
    args = get_default_cpc_config()
    args.arMode, args.nLevelsGRU = "GRU", 1
    torch.manual_seed(3)
    model = CPCModel(getEncoder(args), getAR(args))
    os.makedirs(run_dir)
    path = os.path.join(run_dir, "checkpoint_0.pt")
    save_checkpoint(model.state_dict(), None, None, None, path)
    with open(os.path.join(run_dir, "checkpoint_args.json"), "w") as f:
        json.dump(vars(args), f, indent=2)
    with open(os.path.join(run_dir, "checkpoint_logs.json"), "w") as f:
        json.dump({"epoch": [0]}, f)
    return path


def tool_case(files, seconds, rounds, tmp):
    rng = np.random.RandomState(5)
    src = os.path.join(tmp, "src")
    os.makedirs(src)
    for i in range(files):
        audio.write_wav(os.path.join(src, f"file_{i:05d}.wav"), (rng.randn(1, int(16000 * seconds)) * 3000).astype(np.int16), 16000)
    ckpt = make_checkpoint(os.path.join(tmp, "run"))
    res = dict(files=files, seconds_each=seconds, audio_seconds=files * seconds, rounds=rounds,
               note="PCM16 .wav in and the outputs in a memory-backed directory when there is one; the device is synchronised "
                    "between the stages; the first run of each format (warm-up) is left out")
    for fmt in ("fea", "npy"):
        runs = []
        for r in range(rounds + 1):
            out = os.path.join(tmp, f"out_{fmt}_{r}")
            t0 = time.perf_counter()
            timings = bz.main([src, out, ckpt, "--format", fmt])
            timings["wall"] = time.perf_counter() - t0
            timings["output_bytes"] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
            if r:
                runs.append(timings)
            shutil.rmtree(out)
        res[fmt] = {k + "_s": stats([t[k] for t in runs]) for k in ("wall",) + bz.STAGES}
        res[fmt]["output_bytes"] = runs[0]["output_bytes"]
        res[fmt]["audio_seconds_per_wall_second"] = files * seconds / res[fmt]["wall_s"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_rows", type=int, default=10000)
    ap.add_argument("--no_tool", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("export_bench needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    tmp = tempfile.mkdtemp(prefix="cpc_export_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        if args.quick:
            res["format_rows"] = format_case(2000, 256, 500, 2, tmp)
            if not args.no_tool:
                res["tool"] = tool_case(6, 2.0, 1, tmp)
        else:
            res["format_rows"] = format_case(100000, 256, args.host_rows, args.rounds, tmp)
            if not args.no_tool:
                res["tool"] = tool_case(360, 10.0, 3, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
