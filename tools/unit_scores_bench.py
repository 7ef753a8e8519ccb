#!/usr/bin/env python3
"""Timings of the unit-against-phone counts on one MI355X.  Prints one JSON object and writes it to --out.
Times only: nothing here is a promise.

  1. Workload: --hours (100) hours of 10 ms frames (36 M), utterances of 2 to 35 s, unit streams in runs of mean 3 frames over
     n_units = 50 / 200 / 2000, label streams in runs of mean 8 frames over 41 phones, phone 0 (silence) holding a fifth of the
     frames.  Both packs dense and in the same order, so that the restatements below are one expression each.
  2. Arms, taken in turn for --rounds rounds, device events around each: cpc_unit_counts in the form its shape selects (with the
     memsets of its tables; the LDS form does not fold equal adjacent cells, the global form does), the same in the other
     forms it can take (the LDS form folded, the global form folded and plain), cpc_unit_boundaries, and a plain-torch
     restatement on the device: torch.bincount of the fused index unit * n_phones + label and, for the run starts, `!=` on
     shifted tensors and two more bincounts.  Median, minimum and maximum per arm: the spread over rounds is the three of them.
  3. The host statement: numpy bincount of the same fused index INCLUDING the copy of both packs to the host (wall seconds, once).
  4. The byte floor: 8 bytes per frame (one unit, one label) over the bandwidth MEASURED here in the same run, not a datasheet
     figure: the larger of a torch reduction over a buffer of the workload's size (bytes read) and a torch copy of it (bytes read
     and written).
  5. The tool (cpc2_amd.eval.unit_quality --quantized) on one synthetic hour written to a temporary directory, by stage.
Every arm's tables are checked to equal the numpy statement.

    python tools/unit_scores_bench.py [--hours 100] [--rounds 9] [--out profiles/unit_scores_bench.json]
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
from cpc2_amd.dataset import parseSeqLabels  # noqa: E402
from cpc2_amd.eval import unit_quality as uq  # noqa: E402

DEV = torch.device("cuda:0")
N_PHONES = 41
TOL = 2
LDS, GLOBAL, PLAIN, FOLD = 1, 2, 4, 8


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), rounds=len(ms))


def stream(rng, n, n_symbols, mean_run, p_first=None):
    """n symbols in runs of geometric length; p_first: the probability of symbol 0 per run (the others share the rest)."""
    n_runs = int(n / mean_run * 1.2) + 16
    while True:
        lens = rng.geometric(1.0 / mean_run, size=n_runs)
        if lens.sum() >= n:
            break
        n_runs *= 2
    if p_first is None:
        sym = rng.integers(0, n_symbols, size=n_runs)
    else:
        sym = np.where(rng.random(n_runs) < p_first, 0, rng.integers(1, n_symbols, size=n_runs))
    return np.repeat(sym, lens)[:n].astype(np.int32)


def utterance_lengths(rng, frames):
    out = []
    left = frames
    while left > 0:
        n = int(min(rng.integers(200, 3501), left))
        out.append(n)
        left -= n
    return np.array(out, dtype=np.int32)


class Case:
    def __init__(self, frames, n_units, seed=0):
        rng = np.random.default_rng(seed + n_units)
        self.n_units, self.frames = n_units, frames
        self.lengths_host = utterance_lengths(rng, frames)
        self.u = len(self.lengths_host)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.lengths_host[:-1], dtype=np.int64)]).astype(np.int64)
        self.units = torch.from_numpy(stream(rng, frames, n_units, 3)).to(DEV)
        self.labels = torch.from_numpy(stream(rng, frames, N_PHONES, 8, p_first=0.2)).to(DEV)
        self.offsets = torch.from_numpy(self.offsets_host).to(DEV)
        self.lengths = torch.from_numpy(self.lengths_host).to(DEV)
        self.first = torch.zeros(frames, dtype=torch.bool, device=DEV)
        self.first[self.offsets] = True
        self.joint = torch.zeros(n_units, N_PHONES, dtype=torch.int64, device=DEV)
        self.unit_runs = torch.zeros(n_units, dtype=torch.int64, device=DEV)
        self.phone_runs = torch.zeros(N_PHONES, dtype=torch.int64, device=DEV)
        self.invalid = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.out = torch.empty(self.u, 5, dtype=torch.int32, device=DEV)
        self.lib = _lib.load()
        need = max(self.lib.cpc_unit_counts_scratch_bytes(self.u), self.lib.cpc_unit_boundaries_scratch_bytes(self.u, frames))
        self.scratch = torch.empty(need, dtype=torch.uint8, device=DEV)

    def _args(self):
        p = _lib.ptr
        return (p(self.units), self.frames, p(self.offsets), p(self.labels), self.frames, p(self.offsets), p(self.lengths), self.u)

    def counts(self, form):
        p = _lib.ptr
        for t in (self.joint, self.unit_runs, self.phone_runs, self.invalid):
            t.zero_()
        _lib.check(self.lib.cpc_unit_counts(*self._args(), self.n_units, N_PHONES, form, p(self.joint), p(self.unit_runs),
                                            p(self.phone_runs), p(self.invalid), p(self.scratch), self.scratch.numel(),
                                            _lib.stream_ptr(DEV)), "unit_counts")
        return self.joint, self.unit_runs, self.phone_runs

    def boundaries(self):
        p = _lib.ptr
        _lib.check(self.lib.cpc_unit_boundaries(*self._args(), self.frames, TOL, p(self.out), p(self.scratch), self.scratch.numel(),
                                                _lib.stream_ptr(DEV)), "unit_boundaries")
        return self.out

    def plain_torch(self):
        """The same three tables in plain torch on the device."""
        z, y = self.units.long(), self.labels.long()
        joint = torch.bincount(z * N_PHONES + y, minlength=self.n_units * N_PHONES).view(self.n_units, N_PHONES)
        zs, ys = self.first.clone(), self.first.clone()
        zs[1:] |= self.units[1:] != self.units[:-1]
        ys[1:] |= self.labels[1:] != self.labels[:-1]
        return joint, torch.bincount(z[zs], minlength=self.n_units), torch.bincount(y[ys], minlength=N_PHONES)

    def host(self):
        """numpy on this host's CPU, the copy of both packs included."""
        z, y = self.units.cpu().numpy().astype(np.int64), self.labels.cpu().numpy().astype(np.int64)
        joint = np.bincount(z * N_PHONES + y, minlength=self.n_units * N_PHONES).reshape(self.n_units, N_PHONES)
        first = np.zeros(self.frames, bool)
        first[self.offsets_host] = True
        zs, ys = first.copy(), first.copy()
        zs[1:] |= z[1:] != z[:-1]
        ys[1:] |= y[1:] != y[:-1]
        return joint, np.bincount(z[zs], minlength=self.n_units), np.bincount(y[ys], minlength=N_PHONES)


def measured_bandwidth(nbytes, rounds):
    """Bytes per second of a torch reduction that reads a buffer of nbytes once and of a torch copy that reads and writes it
    (medians over alternating rounds) -> (the larger of the two, both records)."""
    buf = torch.ones(nbytes // 4, dtype=torch.int32, device=DEV)
    dst = torch.empty_like(buf)
    arms = {"sum": lambda: buf.sum(), "copy": lambda: dst.copy_(buf)}
    for fn in arms.values():
        fn()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(once(fn)[0])
    rate = {"sum": nbytes / (float(np.median(ms["sum"])) * 1e-3), "copy": 2 * nbytes / (float(np.median(ms["copy"])) * 1e-3)}
    rec = {k: dict(stats(v), GB_per_s=rate[k] / 1e9) for k, v in ms.items()}
    return max(rate.values()), rec


def run_kernels(frames, rounds):
    lds_cells = _lib.load().cpc_unit_counts_lds_cells()
    bw, bw_ms = measured_bandwidth(frames * 8, rounds)
    out = {"frames": frames, "n_phones": N_PHONES, "tolerance": TOL, "lds_cells": lds_cells, "chunk": _lib.load().cpc_unit_counts_chunk(),
           "measured_GB_per_s": bw / 1e9, "bandwidth_arms": bw_ms, "byte_floor_ms": frames * 8 / bw * 1e3, "shapes": {}}
    for n_units in (50, 200, 2000):
        case = Case(frames, n_units)
        fits = n_units * N_PHONES <= lds_cells
        arms = {"counts": lambda: case.counts(0), "counts_global": lambda: case.counts(GLOBAL),
                "counts_global_plain": lambda: case.counts(GLOBAL | PLAIN), "boundaries": case.boundaries, "plain_torch": case.plain_torch}
        if fits:
            arms["counts_lds_folded"] = lambda: case.counts(LDS | FOLD)
        t0 = time.perf_counter()
        want = case.host()
        host_s = time.perf_counter() - t0
        equal = {}
        for name, fn in arms.items():
            got = fn()
            fn()
            torch.cuda.synchronize()
            if name != "boundaries":
                equal[name] = bool(all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)))
        ms = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                ms[k].append(once(fn)[0])
        rec = {k: stats(v) for k, v in ms.items()}
        rec.update({"utterances": case.u, "selected_form": "lds" if fits else "global", "equals_numpy": equal, "host_numpy_s": host_s,
                    "invalid": int(case.invalid.item()), "mean_unit_run": frames / int(want[1].sum()),
                    "mean_phone_run": frames / int(want[2].sum()), "silence_share": float(want[0][:, 0].sum() / frames),
                    "counts_over_plain_torch": rec["counts"]["median_ms"] / rec["plain_torch"]["median_ms"],
                    "counts_over_byte_floor": rec["counts"]["median_ms"] / out["byte_floor_ms"],
                    "counts_GB_per_s": frames * 8 / (rec["counts"]["median_ms"] * 1e-3) / 1e9,
                    "boundary_totals": [int(v) for v in case.out.sum(dim=0).tolist()]})
        out["shapes"][f"units{n_units}"] = rec
        print(f"n_units={n_units}: {json.dumps(rec)}", file=sys.stderr, flush=True)
        del case, arms
        torch.cuda.empty_cache()
    return out


def run_tool(frames):
    """unit_quality --quantized on a synthetic hour, by stage (wall seconds, the device synchronised at the end of each)."""
    rng = np.random.default_rng(7)
    lengths = utterance_lengths(rng, frames)
    units, labels = stream(rng, frames, 200, 3), stream(rng, frames, N_PHONES, 8, p_first=0.2)
    with tempfile.TemporaryDirectory() as tmp:
        quant, phone = os.path.join(tmp, "quantized_outputs.txt"), os.path.join(tmp, "labels.txt")
        at = 0
        with open(quant, "w") as fq, open(phone, "w") as fp:
            for i, n in enumerate(lengths):
                fq.write(("\n" if i else "") + f"utt{i}\t" + ",".join(map(str, units[at:at + n])))
                fp.write(f"utt{i} " + " ".join(map(str, labels[at:at + n])) + "\n")
                at += n
        t0 = time.perf_counter()
        uq.read_quantized(quant)
        t1 = time.perf_counter()
        parseSeqLabels(phone)
        t2 = time.perf_counter()
        res = uq.main(["--quantized", quant, "--pathPhone", phone, "--out", os.path.join(tmp, "out")])
        torch.cuda.synchronize()
        t3 = time.perf_counter()
    return {"frames": frames, "utterances": len(lengths), "read_quantized_s": t1 - t0, "parse_labels_s": t2 - t1, "whole_tool_s": t3 - t2,
            "counts_scores_and_write_s": (t3 - t2) - (t1 - t0) - (t2 - t1), "pnmi": res["scores"]["pnmi"],
            "bitrate_frames": res["scores"]["bitrate_frames"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_scores_bench.json"))
    args = ap.parse_args()
    frames = int(args.hours * 360000)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernels": run_kernels(frames, args.rounds),
           "tool": run_tool(min(frames, 360000))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
