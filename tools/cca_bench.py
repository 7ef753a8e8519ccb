#!/usr/bin/env python3
"""The streaming second-moment kernel (csrc/moments.hip) and the CCA tool on one MI355X.  Writes profiles/cca_bench.json (and
prints it).

Kernel: n = 2^20 rows at dx = dy = 256, dx = dy = 512 and the one-stream form at 256.  Per shape, timed by device events in
alternating rounds (kernel, torch, kernel, torch, ...), the best round and the spread (max / min over the rounds) of each:
  kernel_ms            cpc_moments_accumulate (both kernels)
  torch_ms             Z.double().T @ Z.double() with Z = cat(x, y): the plain-torch way, which needs an [n, D] f64 copy of the
                       inputs (8 bytes per element, the figure `torch_extra_bytes`) that the kernel never makes
  bytes_floor_ms       one read of the f32 inputs at 8.0 TB/s (HBM3E spec) -- what a kernel that read each input once would take
  useful_tflops        n D (D + 1) flops (the upper triangle, diagonal included, one multiply and one add each) over kernel_ms
  issued_tflops        the flops of the 64 x 64 tiles the kernel actually runs (padding and the full diagonal tiles included)
  frac_of_probe_peak   issued_tflops over the best rate of the stand-alone issue-rate probe tools/mfma_f64_probe.hip, when the
                       probe's binary is given (--probe PATH) or hipcc is there to build it; otherwise "not measured"
Tool: python -m cpc2_amd.cca.train_cca on one synthetic hour (360 files of 10 s of noise, two seeded CPC-small models, hidden
256), seconds by stage: decode, features X, features Y, moments, solve (each stage ends in a device synchronise).

    python tools/cca_bench.py [--reps 5] [--rounds 3] [--probe PATH] [--no-tool]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd.cca import Moments  # noqa: E402

HBM_BPS = 8.0e12
DEV = torch.device("cuda:0")
SHAPES = [(1 << 20, 256, 256), (1 << 20, 512, 512), (1 << 20, 256, 0)]


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


def probe_peak(path):
    """Best TFLOP/s of the issue-rate probe (a child process), or None."""
    tmp = None
    try:
        if path is None:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not os.path.exists(hipcc):
                return None, None
            tmp = tempfile.mkdtemp()
            path = os.path.join(tmp, "mfma_f64_probe")
            subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", os.path.join(ROOT, "tools", "mfma_f64_probe.hip"), "-o", path])
        text = subprocess.run([path], stdout=subprocess.PIPE, text=True, timeout=120, check=True).stdout
        peak = [float(ln.split()[1]) for ln in text.splitlines() if ln.startswith("peak_tflops")]
        return (peak[0] if peak else None), text.splitlines()
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)


def shape_record(n, dx, dy, reps, rounds, peak):
    gen = torch.Generator().manual_seed(n + dx + dy)
    x = torch.randn(n, dx, generator=gen).to(DEV)
    y = torch.randn(n, dy, generator=gen).to(DEV) if dy else None
    D = dx + dy
    m = Moments(dx, dy, device=DEV)

    def mine():
        m.update(x, y)

    def base():
        z = (x if y is None else torch.cat([x, y], dim=1)).double()
        return z.T @ z
    # the results agree (f64 both; the orders of summation differ)
    m.update(x, y)
    ref = base()
    rel = float(((m.gram - ref).abs().max() / ref.abs().max()).item())
    del ref
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(mine, reps))
        b.append(timed(base, reps))
    tiles = (D + 63) // 64
    useful = float(n) * D * (D + 1)
    issued = 2.0 * n * 64 * 64 * tiles * (tiles + 1) / 2
    rec = dict(n=n, dx=dx, dy=dy, kernel_ms=min(a), kernel_spread=max(a) / min(a), torch_ms=min(b), torch_spread=max(b) / min(b),
               kernel_over_torch=min(a) / min(b), torch_extra_bytes=8 * n * D, bytes_floor_ms=4.0 * n * D / HBM_BPS * 1e3,
               useful_tflops=useful / (min(a) * 1e-3) / 1e12, issued_tflops=issued / (min(a) * 1e-3) / 1e12,
               max_rel_difference_to_torch=rel)
    rec["frac_of_probe_peak"] = rec["issued_tflops"] / peak if peak else "not measured"
    return rec


def tool_record(files=360, seconds=10, hidden=256, n_components=100):
    from cpc2_amd import audio
    from cpc2_amd.cca import train_cca
    from cpc2_amd.model import CPCAR, CPCEncoder, CPCModel
    tmp = tempfile.mkdtemp()
    try:
        gen = torch.Generator().manual_seed(0)
        os.makedirs(os.path.join(tmp, "db", "spk"))
        for i in range(files):
            wave = (0.1 * torch.randn(1, seconds * 16000, generator=gen)).clamp(-1, 1)
            audio.write_wav(os.path.join(tmp, "db", "spk", f"f{i:04d}.wav"), (wave * 32767).round().to(torch.int16), 16000)
        paths = []
        for tag, seed in (("X", 1), ("Y", 2)):
            run = os.path.join(tmp, "run" + tag)
            os.makedirs(run)
            torch.manual_seed(seed)
            model = CPCModel(CPCEncoder(hidden), CPCAR(hidden, hidden, False, 1))
            with open(os.path.join(ROOT, "tests", "golden", "ref_checkpoint", "checkpoint_args.json")) as f:
                run_args = json.load(f)
            run_args.update(hiddenEncoder=hidden, hiddenGar=hidden)
            with open(os.path.join(run, "checkpoint_args.json"), "w") as f:
                json.dump(run_args, f)
            with open(os.path.join(run, "checkpoint_logs.json"), "w") as f:
                json.dump({}, f)
            torch.save({"gEncoder": model.state_dict()}, os.path.join(run, "checkpoint_0.pt"))
            paths.append(os.path.join(run, "checkpoint_0.pt"))
        timings = {}
        t0 = time.perf_counter()
        model = train_cca.main(["--path_cp_X", paths[0], "--path_cp_Y", paths[1], "--path_db", os.path.join(tmp, "db"),
                                "--path_output", os.path.join(tmp, "out"), "--n_components", str(n_components)], timings=timings)
        wall = time.perf_counter() - t0
        return dict(files=files, audio_s=files * seconds, hidden=hidden, n_components=n_components, frames=model.n_samples_,
                    n_iter_max=int(max(model.n_iter_)) if len(model.n_iter_) else 0, wall_s=wall,
                    stage_s={k: round(v, 4) for k, v in timings.items()})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--probe", default=None, help="a built tools/mfma_f64_probe.hip (default: built with hipcc, if there)")
    ap.add_argument("--no-tool", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cca_bench.json"))
    a = ap.parse_args()
    peak, probe_lines = probe_peak(a.probe)
    out = dict(device=torch.cuda.get_device_name(0), probe_peak_tflops=peak if peak else "not measured", probe=probe_lines,
               shapes=[])
    t0 = time.perf_counter()
    for n, dx, dy in SHAPES:
        out["shapes"].append(shape_record(n, dx, dy, a.reps, a.rounds, peak))
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
