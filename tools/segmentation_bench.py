#!/usr/bin/env python3
"""Timings of phone-boundary segmentation on one MI355X.  Prints one JSON object and writes it to --out.
Times only: nothing here is a promise.

  1. cpc_seg_dissimilarity and cpc_seg_boundaries on b = 8 and 64 utterances of L = 250 / 1000 / 4096 frames, D = 256 columns,
     K = 30 thresholds (0.01 .. 0.30), tolerance 2, reference boundaries from random labels with segments of 3 to 12 frames
     (features x_t = 0.8 x_t-1 + e_t): device events around one launch each, the configurations taken in turn for --rounds
     rounds; median, minimum and maximum per configuration.
  2. The same batches through (a) tests/segmentation_oracle.py, the numpy float64 / plain Python statement on this host's CPU,
     INCLUDING the copy of the features to the host (wall seconds, once), checked to return the kernels' peaks and counts where
     its margin calls the case clear, and (b) a plain-torch restatement of step 1 on the device (float64 products and sums, one
     launch per step; device events, --rounds rounds), checked against the kernel within the oracle's bound.

    python tools/segmentation_bench.py [--rounds 15] [--out profiles/segmentation_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segmentation_oracle as SO  # noqa: E402
from cpc2_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
D = 256
THRESHOLDS = [round(0.01 * i, 2) for i in range(1, 31)]
TOL = 2


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), rounds=len(ms))


class Case:
    """One packed batch and its output buffers; dissimilarity() and boundaries() are one launch each (the first also clears the
    status words with a memset)."""

    def __init__(self, b, length, seed=0):
        rng = np.random.default_rng(seed + 1000 * b + length)
        e = rng.standard_normal((b, length, D)).astype(np.float32)
        x = np.empty_like(e)
        x[:, 0] = e[:, 0]
        for t in range(1, length):
            x[:, t] = np.float32(0.8) * x[:, t - 1] + e[:, t]
        self.b, self.length, self.total = b, length, b * length
        self.host = x.reshape(self.total, D)
        self.x = torch.from_numpy(self.host).to(DEV)
        self.refs = []
        for _ in range(b):
            cuts = np.cumsum(rng.integers(3, 13, size=length))
            self.refs.append(cuts[cuts < length].astype(np.int32))
        cnt = np.array([len(r) for r in self.refs], dtype=np.int32)
        self.total_ref = int(cnt.sum())
        self.ref = torch.from_numpy(np.concatenate(self.refs)).to(DEV)
        self.ref_off = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.int64)).to(DEV)
        self.ref_cnt = torch.from_numpy(cnt).to(DEV)
        self.offsets = (torch.arange(b, dtype=torch.int64) * length).to(DEV)
        self.lengths = torch.full((b,), length, dtype=torch.int32, device=DEV)
        self.thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device=DEV)
        self.d = torch.empty(self.total, dtype=torch.float64, device=DEV)
        self.status1 = torch.empty(b, dtype=torch.int32, device=DEV)
        self.n_peaks = torch.empty(b, dtype=torch.int32, device=DEV)
        self.pos = torch.empty(self.total, dtype=torch.int32, device=DEV)
        self.prom = torch.empty(self.total, dtype=torch.float64, device=DEV)
        self.range = torch.empty(b, dtype=torch.float64, device=DEV)
        self.counts = torch.empty(b, len(THRESHOLDS), 4, dtype=torch.int32, device=DEV)
        self.status2 = torch.empty(b, dtype=torch.int32, device=DEV)
        self.lib = _lib.load()

    def dissimilarity(self):
        p = _lib.ptr
        _lib.check(self.lib.cpc_seg_dissimilarity(p(self.x), self.total, D, D, p(self.offsets), p(self.lengths), self.b, self.length,
                                                  p(self.d), p(self.status1), _lib.stream_ptr(DEV)), "seg_dissimilarity")

    def boundaries(self):
        p = _lib.ptr
        _lib.check(self.lib.cpc_seg_boundaries(p(self.d), self.total, p(self.offsets), p(self.lengths), self.b, p(self.thr),
                                               len(THRESHOLDS), p(self.ref), self.total_ref, p(self.ref_off), p(self.ref_cnt), None, TOL,
                                               p(self.n_peaks), p(self.pos), p(self.prom), p(self.range), p(self.counts),
                                               p(self.status2), _lib.stream_ptr(DEV)), "seg_boundaries")

    def torch_dissimilarity(self):
        """Step 1 in plain torch on the device: float64 products and sums, d [b, L - 1]."""
        x = self.x.view(self.b, self.length, D).double()
        norm = (x * x).sum(-1)
        dot = (x[:, :-1] * x[:, 1:]).sum(-1)
        prod = norm[:, :-1] * norm[:, 1:]
        return torch.where(prod != 0, 1.0 - dot / torch.sqrt(prod), torch.ones_like(prod))


def run(rounds):
    out = {"dim": D, "thresholds": len(THRESHOLDS), "tolerance": TOL, "lds_entries": _lib.load().cpc_seg_lds_entries(), "shapes": {}}
    for b in (8, 64):
        for length in (250, 1000, 4096):
            case = Case(b, length)
            arms = {"dissimilarity": case.dissimilarity, "boundaries": case.boundaries, "plain_torch_dissimilarity": case.torch_dissimilarity}
            for fn in arms.values():
                fn()
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(rounds):
                for k, fn in arms.items():
                    ms[k].append(once(fn)[0])
            rec = {k: stats(v) for k, v in ms.items()}
            rec["feature_MB"] = case.total * D * 4 / 2 ** 20
            rec["dissimilarity_GB_per_s"] = case.total * D * 4 / (rec["dissimilarity"]["median_ms"] * 1e-3) / 1e9
            rec["peaks"] = int(case.n_peaks.sum())
            rec["status_ok"] = bool((case.status1 == 0).all() and (case.status2 == 0).all())
            dk = case.d.view(b, length)[:, :length - 1]
            rec["plain_torch_max_abs_diff"] = float((case.torch_dissimilarity() - dk).abs().max())
            rec["bound"] = SO.dissimilarity_bound(D)
            # the float64 statement on the host, the copy of the features included
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = case.x.cpu().numpy().reshape(b, length, D)
            wants, margins = [], []
            for i in range(b):
                d, _ = SO.dissimilarity(host[i])
                wants.append(SO.segment(d, THRESHOLDS, ref=case.refs[i].tolist(), tol=TOL))
            rec["host_oracle_s"] = time.perf_counter() - t0
            for i in range(b):
                margins.append(SO.margin(SO.dissimilarity(host[i])[0], THRESHOLDS))
            pos, n_peaks, counts = case.pos.cpu().numpy(), case.n_peaks.cpu().numpy(), case.counts.cpu().numpy()
            clear = [i for i in range(b) if margins[i] >= 1e-9]
            rec["clear_cases"] = len(clear)
            rec["smallest_margin"] = float(min(margins))
            rec["host_equal"] = bool(all(pos[i * length:i * length + n_peaks[i]].tolist() == wants[i]["peaks"] and
                                         counts[i].tolist() == wants[i]["counts"] for i in clear))
            out["shapes"][f"b{b}_L{length}"] = rec
            print(f"b={b} L={length}: {json.dumps(rec)}", file=sys.stderr, flush=True)
            del case
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmentation_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernels": run(args.rounds)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
