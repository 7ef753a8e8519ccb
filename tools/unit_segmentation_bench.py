#!/usr/bin/env python3
"""Timings of duration-penalized unit segmentation on one MI355X.  Prints one JSON object and writes it to
--out.  Times only: nothing here is a promise.

  1. Workload: --hours (1) hour of 10 ms frames (360 000), utterances of 2 to 35 s packed densely, costs for K = 50 / 200 / 2000
     codes: uniform in [2, 6) with a planted unit stream in runs of mean 6 frames whose cost is 2 lower, the penalties spread over
     [0, 4].  1 and 8 penalties per launch.
  2. Arms, taken in turn for --rounds rounds, device events around each: cpc_segment_units (prefix, recurrence and backtrace: the
     whole entry point) with 1 and with 8 penalties, and a plain-torch restatement on the device with one penalty: per frame one
     set of launches over all utterances at once (gather the frame's rows, compare, where, add, min), then per frame the
     backtrace.  Median, minimum and maximum per arm: the spread over rounds is the three of them.
  3. The host statement: the numpy float64 program of the definition, utterance after utterance, INCLUDING the copy of the cost
     matrix to the host (wall seconds, once, one penalty).
  4. The byte floor: frames * K * 4 bytes read once, over the read bandwidth MEASURED here in the same run (a torch reduction over
     a buffer of the workload's size), not a datasheet figure.  The time loop is a dependency chain, so the floor is far away by
     construction; the frames-per-second figure is the one to read.
  5. The tool (cpc2_amd.clustering.segment_quantization --time_stages) on the repository's audio fixture with a codebook made by
     clustering_script, by stage.  Nine short files: a measurement of overheads, stated as such.
Every arm's units are checked to equal the numpy statement.

    python tools/unit_segmentation_bench.py [--hours 1] [--rounds 7] [--out profiles/unit_segmentation_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import unit_dp_oracle as DO  # noqa: E402
from cpc2_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
PENALTIES = [1.0, 0.0, 0.25, 0.5, 1.5, 2.0, 3.0, 4.0]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), rounds=len(ms))


def utterance_lengths(rng, frames):
    out, left = [], frames
    while left > 0:
        n = int(min(rng.integers(200, 3501), left))
        out.append(n)
        left -= n
    return np.array(out, dtype=np.int32)


class Case:
    def __init__(self, frames, k, seed=0):
        rng = np.random.default_rng(seed + k)
        self.k, self.frames = k, frames
        self.lengths_host = utterance_lengths(rng, frames)
        self.u = len(self.lengths_host)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.lengths_host[:-1], dtype=np.int64)]).astype(np.int64)
        n_runs = frames // 6 * 2 + 64
        planted = np.repeat(rng.integers(0, k, size=n_runs), rng.geometric(1.0 / 6, size=n_runs))[:frames]
        assert len(planted) == frames
        gen = torch.Generator(device=DEV).manual_seed(seed + k)
        self.cost = torch.rand(frames, k, device=DEV, generator=gen) * 4 + 2
        self.cost[torch.arange(frames, device=DEV), torch.from_numpy(planted).to(DEV)] -= 2
        self.offsets = torch.from_numpy(self.offsets_host).to(DEV)
        self.lengths = torch.from_numpy(self.lengths_host).to(DEV)
        self.buffers = {}

    def kernel(self, pens):
        """The raw entry point into buffers made once per number of penalties: no allocation and no copy in the timed region."""
        lib, p, n_pen = _lib.load(), _lib.ptr, len(pens)
        if n_pen not in self.buffers:
            need = lib.cpc_segment_units_scratch_bytes(self.u, self.frames, self.k, n_pen)
            self.buffers[n_pen] = (torch.full((n_pen, self.frames), -1, dtype=torch.int32, device=DEV),
                                   torch.zeros(n_pen, self.u, dtype=torch.float64, device=DEV),
                                   torch.zeros(n_pen, self.u, dtype=torch.int32, device=DEV),
                                   torch.zeros(n_pen, self.u, dtype=torch.int32, device=DEV),
                                   torch.empty(need, dtype=torch.uint8, device=DEV))
        units, energy, n_seg, status, scratch = self.buffers[n_pen]
        pen = np.asarray(pens, dtype=np.float64)
        _lib.check(lib.cpc_segment_units(p(self.cost), self.frames, self.k, self.k, p(self.offsets), p(self.lengths), self.u,
                                         pen.ctypes.data, n_pen, p(units), p(energy), p(n_seg), p(status), p(scratch), scratch.numel(),
                                         _lib.stream_ptr(DEV)), "segment_units")
        return units, energy, n_seg, status

    def plain_torch(self, lam):
        """The definition in plain torch on the device, all utterances at once, one set of launches per frame."""
        t_max = int(self.lengths_host.max())
        off, length = self.offsets, self.lengths.long()
        rows = torch.arange(self.u, device=DEV)
        lam = torch.tensor(lam, dtype=torch.float64, device=DEV)
        V = self.cost[off].double()
        a = torch.zeros(t_max, self.u, dtype=torch.int64, device=DEV)
        stay = torch.ones(t_max, self.u, self.k, dtype=torch.bool, device=DEV)
        m, a[0] = V.min(dim=1)
        for t in range(1, t_max):
            live = (length > t).unsqueeze(1)
            sw = (m + lam).unsqueeze(1)
            stay[t] = V <= sw
            new = self.cost[off + torch.clamp(length - 1, max=t)].double() + torch.where(stay[t], V, sw)
            V = torch.where(live, new, V)
            m, a[t] = V.min(dim=1)
        units = torch.full((self.frames,), -1, dtype=torch.int32, device=DEV)
        u = a[length - 1, rows]
        for t in range(t_max - 1, -1, -1):
            live = length > t
            units[(off + t)[live]] = u[live].int()
            if t >= 1:
                u = torch.where(live & ~stay[t, rows, u], a[t - 1], u)
        return units

    def host(self, lam):
        """numpy on this host's CPU, the copy of the cost matrix included."""
        cost = self.cost.cpu().numpy()
        return DO.segment_pack(cost, self.offsets_host, self.lengths_host, [lam])


def measured_read_bandwidth(nbytes, rounds):
    buf = torch.ones(nbytes // 4, dtype=torch.float32, device=DEV)
    buf.sum()
    ms = [once(lambda: buf.sum())[0] for _ in range(rounds)]
    return nbytes / (float(np.median(ms)) * 1e-3), stats(ms)


def run_kernels(frames, rounds):
    out = {"frames": frames, "wave_k": _lib.load().cpc_segment_units_wave_k(), "penalties": PENALTIES, "shapes": {}}
    for k in (50, 200, 2000):
        case = Case(frames, k)
        bw, bw_ms = measured_read_bandwidth(frames * k * 4, rounds)
        floor_ms = frames * k * 4 / bw * 1e3
        arms = {"kernel_1_penalty": lambda: case.kernel(PENALTIES[:1]), "kernel_8_penalties": lambda: case.kernel(PENALTIES),
                "plain_torch_1_penalty": lambda: case.plain_torch(PENALTIES[0])}
        t0 = time.perf_counter()
        want = case.host(PENALTIES[0])
        host_s = time.perf_counter() - t0
        one, eight, plain = (fn() for fn in arms.values())
        torch.cuda.synchronize()
        equal = {"kernel_1_penalty": bool(np.array_equal(one[0][0].cpu().numpy(), want[0][0])
                                          and np.array_equal(one[1][0].cpu().numpy(), want[1][0])),
                 "kernel_8_penalties_row_0": bool(np.array_equal(eight[0][0].cpu().numpy(), want[0][0])),
                 "plain_torch_1_penalty": bool(np.array_equal(plain.cpu().numpy(), want[0][0]))}
        ms = {name: [] for name in arms}
        for _ in range(rounds):
            for name, fn in arms.items():
                ms[name].append(once(fn)[0])
        rec = {name: stats(v) for name, v in ms.items()}
        k1, k8 = rec["kernel_1_penalty"]["median_ms"], rec["kernel_8_penalties"]["median_ms"]
        rec.update({"utterances": case.u, "longest_utterance": int(case.lengths_host.max()),
                    "form": "wave" if k <= out["wave_k"] else "workgroup", "equals_numpy": equal, "host_numpy_s": host_s,
                    "segments": [int(v) for v in eight[2].sum(dim=1).tolist()], "measured_read_GB_per_s": bw / 1e9,
                    "bandwidth_arm": bw_ms, "byte_floor_ms": floor_ms,
                    "frames_per_s_1_penalty": frames / (k1 * 1e-3), "frame_penalties_per_s_8_penalties": 8 * frames / (k8 * 1e-3),
                    "plain_torch_over_kernel": rec["plain_torch_1_penalty"]["median_ms"] / k1,
                    "host_numpy_over_kernel": host_s * 1e3 / k1, "kernel_over_byte_floor": k1 / floor_ms,
                    "eight_penalties_over_one": k8 / k1})
        out["shapes"][f"k{k}"] = rec
        print(f"k={k}: {json.dumps(rec)}", file=sys.stderr, flush=True)
        del case, arms, one, eight, plain
        torch.cuda.empty_cache()
    return out


def run_tool():
    """segment_quantization on the repository's audio fixture, by stage (wall seconds, the device synchronised after each)."""
    import logging
    import random

    from cpc2_amd.clustering import clustering_script as S
    from cpc2_amd.clustering import segment_quantization as SQ
    golden = os.path.join(ROOT, "tests", "golden")
    ckpt, db = os.path.join(golden, "ref_checkpoint", "checkpoint_7.pt"), os.path.join(golden, "test_db")
    with tempfile.TemporaryDirectory() as tmp:
        random.seed(7)
        torch.manual_seed(7)
        S.main([ckpt, os.path.join(tmp, "clust"), db, "-k", "12", "-n", "2", "--save"])
        for name in ("Kmean", "DPMean"):
            for h in list(logging.getLogger(name).handlers):
                h.close()
                logging.getLogger(name).removeHandler(h)
        last = os.path.join(tmp, "clust", "checkpoint_last.pt")
        SQ.main([last, db, os.path.join(tmp, "warm"), "--penalty", "0", "1"])
        t0 = time.perf_counter()
        log = SQ.main([last, db, os.path.join(tmp, "seg"), "--penalty"] + [str(v) for v in PENALTIES] + ["--time_stages"])
        whole = time.perf_counter() - t0
    return {"files": log["n_files"], "frames": log["n_frames"], "n_units": log["n_units"], "penalties": len(PENALTIES),
            "whole_tool_s": whole, "stages_s": log["seconds"], "mean_min_distance": log["mean_min_distance"],
            "segments": [p["segments"] for p in log["penalties"]],
            "note": "nine short files: set-up (model and codebook loading) and per-file overheads, not throughput"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_segmentation_bench.json"))
    args = ap.parse_args()
    frames = int(args.hours * 360000)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernels": run_kernels(frames, args.rounds),
           "tool": run_tool()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
