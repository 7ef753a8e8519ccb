#!/usr/bin/env python3
"""The window-moments kernel (csrc/seqmoments.hip) and the fit tool of cpc2_amd.dim_reduction on one MI355X.  Writes
profiles/dim_reduction_bench.json (and prints it).  Nothing is gated on these numbers.

Kernel: x [b, s, d] with skip = 1 (SFALinear.update) at the shapes of SHAPES.  Per shape, timed by device events in alternating
rounds (kernel, two calls, broadcast, kernel, ...), the best round and the spread (max / min over the rounds) of each:
  kernel_ms            cpc_seq_moments_accumulate (both kernels): sums, gram and dgram in one pass over x
  two_calls_ms         the same totals from what was there before: x[:, 1:].contiguous() and the f32 difference tensor made by torch,
                       then cpc_moments_accumulate on each (the difference is then rounded to f32, and `two_calls_extra_bytes` are
                       written and read again)
  broadcast_ms         the reference's update in plain torch, f32: two [N, k, k] broadcasts summed over N (only where the
                       [N, k, k] tensor stays under 1 GiB; otherwise "not run")
  bytes_floor_ms       one read of x at 8.0 TB/s (HBM3E spec)
  issued_tflops        the flops of the 64 x 64 tiles the kernel runs, levels and differences (padding and full diagonal tiles included)
  frac_of_probe_peak   issued_tflops over the best rate of tools/mfma_f64_probe.hip, when the probe's binary is given (--probe PATH)
                       or hipcc is there to build it; otherwise "not measured"
Tool: python -m cpc2_amd.dim_reduction --mode SFA on one synthetic hour (360 files of 10 s of noise, one seeded CPC-small model,
hidden 256), seconds by stage: load (listing, decoding, the loader), fit (model, moments, solve), write.

    python tools/dim_reduction_bench.py [--reps 5] [--rounds 3] [--probe PATH] [--no-tool]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cca_bench import probe_peak, timed  # noqa: E402
from cpc2_amd import dim_reduction as DR  # noqa: E402
from cpc2_amd.cca import Moments  # noqa: E402

HBM_BPS = 8.0e12
DEV = torch.device("cuda:0")
SHAPES = [(8, 128, 256), (64, 128, 256), (8192, 128, 256), (4096, 128, 512)]
BROADCAST_LIMIT = 1 << 30


def shape_record(b, s, d, reps, rounds, peak):
    gen = torch.Generator().manual_seed(b + s + d)
    x = torch.randn(b, s, d, generator=gen).to(DEV)
    sfa = DR.SFALinear(d).to(DEV)
    levels, speeds = Moments(d, device=DEV), Moments(d, device=DEV)

    def mine():
        sfa.update(x)

    def two_calls():
        kept = x[:, 1:]
        levels.update(kept.contiguous())
        speeds.update((kept[:, 1:] - kept[:, :-1]).contiguous())

    def broadcast():
        kept = x[:, 1:]
        xt = (kept[:, 1:] - kept[:, :-1]).contiguous().view(-1, d)
        a = (xt.view(-1, 1, d) * xt.view(-1, d, 1)).sum(dim=0)
        xp = kept.contiguous()
        return a, (xp.view(-1, 1, d) * xp.view(-1, d, 1)).sum(dim=0), kept.sum(dim=0).sum(dim=0), (kept ** 2).sum(dim=0).sum(dim=0)

    runs_broadcast = 4 * b * (s - 1) * d * d <= BROADCAST_LIMIT
    # the totals agree (the two-call way rounds each difference to f32 first)
    mine()
    two_calls()
    rel_gram = float(((sfa.gram - levels.gram).abs().max() / levels.gram.abs().max()).item())
    rel_dgram = float(((sfa.dgram - speeds.gram).abs().max() / speeds.gram.abs().max()).item())
    ta, tb, tc = [], [], []
    for _ in range(rounds):
        ta.append(timed(mine, reps))
        tb.append(timed(two_calls, reps))
        if runs_broadcast:
            tc.append(timed(broadcast, reps))
    n = b * s
    tiles = (d + 63) // 64
    issued = 2 * 2.0 * n * 64 * 64 * tiles * (tiles + 1) / 2
    rec = dict(b=b, s=s, d=d, skip=1, kernel_ms=min(ta), kernel_spread=max(ta) / min(ta), two_calls_ms=min(tb),
               two_calls_spread=max(tb) / min(tb), kernel_over_two_calls=min(ta) / min(tb),
               two_calls_extra_bytes=4 * (b * (s - 1) * d + b * (s - 2) * d), bytes_floor_ms=4.0 * n * d / HBM_BPS * 1e3,
               issued_tflops=issued / (min(ta) * 1e-3) / 1e12, max_rel_difference_gram=rel_gram, max_rel_difference_dgram=rel_dgram)
    if runs_broadcast:
        rec.update(broadcast_ms=min(tc), broadcast_spread=max(tc) / min(tc), kernel_over_broadcast=min(ta) / min(tc),
                   broadcast_extra_bytes=2 * 4 * b * (s - 1) * d * d)
    else:
        rec["broadcast_ms"] = "not run"
    rec["frac_of_probe_peak"] = rec["issued_tflops"] / peak if peak else "not measured"
    return rec


def tool_record(files=360, seconds=10, hidden=256):
    from cpc2_amd import audio
    from cpc2_amd.model import CPCAR, CPCEncoder, CPCModel
    tmp = tempfile.mkdtemp()
    try:
        gen = torch.Generator().manual_seed(0)
        os.makedirs(os.path.join(tmp, "db", "spk", "chapter"))
        for i in range(files):
            wave = (0.1 * torch.randn(1, seconds * 16000, generator=gen)).clamp(-1, 1)
            audio.write_wav(os.path.join(tmp, "db", "spk", "chapter", f"f{i:04d}.wav"), (wave * 32767).round().to(torch.int16), 16000)
        run = os.path.join(tmp, "run")
        os.makedirs(run)
        torch.manual_seed(1)
        model = CPCModel(CPCEncoder(hidden), CPCAR(hidden, hidden, False, 1))
        with open(os.path.join(ROOT, "tests", "golden", "ref_checkpoint", "checkpoint_args.json")) as f:
            run_args = json.load(f)
        run_args.update(hiddenEncoder=hidden, hiddenGar=hidden)
        with open(os.path.join(run, "checkpoint_args.json"), "w") as f:
            json.dump(run_args, f)
        with open(os.path.join(run, "checkpoint_logs.json"), "w") as f:
            json.dump({}, f)
        torch.save({"gEncoder": model.state_dict()}, os.path.join(run, "checkpoint_0.pt"))
        timings = {}
        t0 = time.perf_counter()
        sfa = DR.main([os.path.join(run, "checkpoint_0.pt"), os.path.join(tmp, "sfa.pt"), "--pathDB", os.path.join(tmp, "db"),
                       "--extension", ".wav", "--mode", "SFA"], timings=timings)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return dict(files=files, audio_s=files * seconds, hidden=hidden, batchSize=8, sizeWindow=20480, frames_counted=sfa.N_x,
                    frames_summed=sfa.rows_summed, wall_s=wall, stage_s={k: round(v, 4) for k, v in timings.items()})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--probe", default=None, help="a built tools/mfma_f64_probe.hip (default: built with hipcc, if there)")
    ap.add_argument("--no-tool", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dim_reduction_bench.json"))
    a = ap.parse_args()
    peak, probe_lines = probe_peak(a.probe)
    out = dict(device=torch.cuda.get_device_name(0), probe_peak_tflops=peak if peak else "not measured", probe=probe_lines,
               shapes=[])
    t0 = time.perf_counter()
    for b, s, d in SHAPES:
        out["shapes"].append(shape_record(b, s, d, a.reps, a.rounds, peak))
    if not a.no_tool:
        out["tool"] = tool_record()
    out["wall_s"] = time.perf_counter() - t0
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
