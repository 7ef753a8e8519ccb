#!/usr/bin/env python3
"""Spoken term discovery on one MI355X (cpc2_amd/term_discovery.py, csrc/lalign.hip): the local-alignment kernel on a seeded
synthetic hour, against cpc_sdtw on a work list of the same cells, a plain-torch restatement, the numpy statement and two floors.

Workload: --utts (360) utterances of 300..1 500 frames, D = 256 Gaussian frames (rows normalised for the cosine distance), every
unordered pair, both distances; theta a little below the typical distance and a small gamma (the values of the tests' real-valued
family at D = 256), so that paths are long and take steps of all three kinds.

  kernel       device events around local_alignment's kernel call (run_segments) and, in the same rounds, around cpc_sdtw on the
               SAME work list (row item as the query, column items as the documents: the same cells, strips and tiles): the four
               (kernel, distance) arms in alternating rounds after a warm-up of all; every round's time is listed, with the smallest
               and the spread (max - min) / min.  The local alignment carries one more word per cell and a best per lane; there is
               no acceptance ratio, the cells per second of both are written down
  floors       (a) the distance multiply-adds (cells x D) at the unpacked f32 FMA rate of DESIGN.md section 11, 78.6 TFLOP/s;
               (b) the DP alone: lalign.hip built with the distance tile skipped (CPC_SDTW_SKIP_DISTANCES, a probe build made by
               this tool into --probe_lib; stand-in distances 0..15 against theta = 8, gamma = 1), on the same work list
  torch        the same definition in plain torch on the device, on a subset (--torch_rows x --torch_cols): one matmul + acos (or
               cdist) per row item against its padded column items and the DP by anti-diagonals; wall time behind a synchronise
  numpy        the float64 statement of tests/lalign_oracle.py on the host on --numpy_pairs pairs of the shortest utterances,
               the copy of their frames included; its scores and spans are compared with the kernel's
  tool         python -m cpc2_amd.eval.term_discovery from_pre_computed on a synthetic hour of .npy files (--utts files of
               1 000 frames with 50 planted fragments and frame labels): its wall time by stage, from discovery_log.json

Prints one JSON line and writes it to --out (default profiles/term_discovery_bench.json).
    python tools/term_discovery_bench.py [--build_probe_only]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cpc2_amd import _lib  # noqa: E402
from cpc2_amd import build as lib_build  # noqa: E402
from cpc2_amd import term_detection as td  # noqa: E402
from cpc2_amd import term_discovery as tdisc  # noqa: E402
from cpc2_amd.eval import term_discovery as tool  # noqa: E402
from tests import lalign_oracle as L  # noqa: E402

FMA_RATE = 78.6e12 / 2             # unpacked f32 FMAs per second (78.6 TFLOP/s)
PARAMS = {"cosine": (0.49, 0.01), "euclidian": (22.0, 0.3)}       # theta, gamma at D = 256
PROBE_PARAMS = (8.0, 1.0)


def build_probe(path):
    """lalign.hip with the distance tile skipped, as a library of its own (same entry points)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        stub = os.path.join(tmp, "stub.cpp")
        with open(stub, "w") as f:
            f.write("namespace cpc { void set_error(const char *, ...) {} }\n")
        cmd = ([lib_build.HIPCC] + lib_build.FLAGS + lib_build.DEVICE_FLAGS + lib_build.FILE_FLAGS["lalign.hip"]
               + ["-DCPC_SDTW_SKIP_DISTANCES", "-shared", "-x", "hip", os.path.join(lib_build.CSRC, "lalign.hip"), stub, "-o", path])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        noise = [ln for ln in res.stdout.splitlines() if ln.strip() and "is not a recognized feature for this target" not in ln]
        if res.returncode != 0:
            raise RuntimeError("probe build failed:\n" + "\n".join(noise))
    return path


def synthetic(a, distance, dev):
    rng = np.random.default_rng(a.seed)
    lens = rng.integers(300, 1501, a.utts)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    frames = torch.randn(int(lens.sum()), a.dim, device=dev, generator=gen)
    if distance == "cosine":
        frames /= frames.norm(dim=1, keepdim=True)
    off = np.concatenate([[0], np.cumsum(lens[:-1])])
    return frames, torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), lens


class Plan:
    """A work list on the device and what it counts."""

    def __init__(self, lens, plan, dev, rows=None):
        self.seg_a, self.seg_start, self.pair_b, self.pair_a = plan
        if rows is not None:                                       # a plan_segments list: the pair's row item by position
            self.pair_a = np.asarray(rows)[self.pair_a]
        a_len, b_len = lens[self.pair_a], lens[self.pair_b]
        self.cells = int((a_len * b_len).sum())
        self.max_a, self.max_b = int(lens[self.seg_a].max()), int(b_len.max())
        self.dev_lists = [torch.from_numpy(x).to(dev) for x in (self.seg_a, self.seg_start, self.pair_b)]

    def lalign(self, frames, off, lens_d, code, theta, gamma):
        return tdisc.run_segments(frames, off, lens_d, *self.dev_lists, self.max_a, self.max_b, code, theta, gamma)

    def sdtw(self, frames, off, lens_d, code):
        return td.run_segments(frames, off, lens_d, *self.dev_lists, self.max_a, self.max_b, code)


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / 1e3


def probe_run(lib, plan, frames, off, lens_d, code):
    """The probe library on the same work list: seconds between device events."""
    dev = frames.device
    nbytes = lib.cpc_local_align_scratch_bytes(len(plan.seg_a), plan.max_a, plan.max_b)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    score = torch.empty(len(plan.pair_b), dtype=torch.float32, device=dev)
    span = torch.empty(len(plan.pair_b), 5, dtype=torch.int32, device=dev)

    def call():
        status = lib.cpc_local_align(_lib.ptr(frames), frames.size(1), _lib.ptr(off), _lib.ptr(lens_d), int(lens_d.numel()),
                                     *[_lib.ptr(x) for x in plan.dev_lists], len(plan.seg_a), plan.max_a, plan.max_b, code,
                                     PROBE_PARAMS[0], PROBE_PARAMS[1], _lib.ptr(score), _lib.ptr(span), _lib.ptr(scratch), nbytes,
                                     _lib.stream_ptr(dev))
        if status != 0:
            raise RuntimeError(f"probe cpc_local_align failed ({status})")
    call()
    torch.cuda.synchronize()
    return [event_time(call)[1] for _ in range(3)]


def torch_local_align(frames, a_off, a_len, b_offs, b_lens, distance, theta, gamma):
    """The definition in plain torch for one row item against a batch of column items: (score [B], span [B, 5]).  Distances by one
    matmul + acos (cosine) or cdist; DP by anti-diagonals, a cell per (column item, row)."""
    dev = frames.device
    B, n, M = len(b_offs), int(a_len), int(max(b_lens))
    q = frames[a_off:a_off + n]
    x = torch.zeros(B, M, frames.size(1), device=dev)
    for b, (o, m) in enumerate(zip(b_offs, b_lens)):
        x[b, :m] = frames[o:o + m]
    if distance == "cosine":
        d = torch.acos(torch.clamp(torch.matmul(x, q.t()), -1, 1)).transpose(1, 2) / np.pi            # [B, n, M]
    else:
        d = torch.cdist(q.unsqueeze(0).expand(B, n, -1), x)
    valid = torch.arange(M, device=dev).view(1, 1, -1) < torch.tensor(b_lens, device=dev).view(-1, 1, 1)
    d = torch.where(valid, d, torch.full_like(d, float("inf")))
    T = n + M - 1
    rows = torch.arange(n, device=dev)
    skew = torch.full((B, n, T), float("inf"), device=dev)                                           # skew[b, i, t] = d[b, i, t - i]
    skew[:, rows.view(-1, 1), rows.view(-1, 1) + torch.arange(M, device=dev).view(1, -1)] = d
    ninf = torch.full((B, n), float("-inf"), device=dev)                                             # outside the matrix
    zero = torch.zeros(B, n, dtype=torch.long, device=dev)
    p1h, p1l, p1s, p2h, p2l, p2s = ninf, zero, zero, ninf, zero, zero
    best_h = torch.zeros(B, n, device=dev)
    best_j, best_l, best_s = zero.clone(), zero.clone(), zero.clone()
    theta_t, gamma_t = torch.tensor(theta, dtype=torch.float32, device=dev), torch.tensor(gamma, dtype=torch.float32, device=dev)

    def down(t, fill):                                         # value of row i - 1 at row i
        return torch.cat([fill[:, :1], t[:, :-1]], dim=1)

    for t in range(T):
        dc = skew[:, :, t]
        g = theta_t - dc
        cu, up_l, up_s = down(p1h, ninf) - gamma_t, down(p1l, zero), down(p1s, zero)
        cd, dg_l, dg_s = down(p2h, ninf), down(p2l, zero), down(p2s, zero)
        cl = p1h - gamma_t
        use_dg = (cd >= cl) & (cd >= cu)
        use_lf = ~use_dg & (cl >= cu)
        bh = torch.where(use_dg, cd, torch.where(use_lf, cl, cu))
        bl = torch.where(use_dg, dg_l, torch.where(use_lf, p1l, up_l))
        bs = torch.where(use_dg, dg_s, torch.where(use_lf, p1s, up_s))
        opens = bh <= 0
        here = (rows << 16) | (t - rows).clamp(min=0)
        h = torch.where(opens, g, g + bh)
        nl = torch.where(opens, torch.ones_like(bl), bl + 1)
        ns = torch.where(opens, here.view(1, -1).expand(B, -1), bs)
        pos = h > 0
        better = pos & (h > best_h)
        best_h = torch.where(better, h, best_h)
        best_j = torch.where(better, (t - rows).view(1, -1).expand(B, -1), best_j)
        best_l, best_s = torch.where(better, nl, best_l), torch.where(better, ns, best_s)
        nh = torch.where(pos, h, torch.where(torch.isinf(dc), ninf, torch.zeros_like(h)))
        p2h, p2l, p2s, p1h, p1l, p1s = p1h, p1l, p1s, nh, nl, ns
    score = best_h.max(dim=1)[0]
    row = (best_h == score.view(-1, 1)).to(torch.int64).argmax(dim=1)                                # the first row among equals
    pick = row.view(-1, 1)
    s, j, length = best_s.gather(1, pick).view(-1), best_j.gather(1, pick).view(-1), best_l.gather(1, pick).view(-1)
    span = torch.stack([s >> 16, row, s & 0xffff, j, length], dim=1)
    span = torch.where((score > 0).view(-1, 1), span, torch.full_like(span, -1))
    return score, span.to(torch.int32)


def synthetic_hour(a, root):
    """--utts utterances of 1 000 frames as .npy with 50 fragments of 50..150 frames planted in pairs of them (a noisy copy), and
    frame labels (random runs; a fragment carries its labels along): (feature dir, label file)."""
    rng = np.random.default_rng(a.seed + 1)
    feat = os.path.join(root, "features")
    os.makedirs(feat)
    utts = [rng.standard_normal((1000, a.dim)).astype(np.float32) for _ in range(a.utts)]
    labels = []
    for _ in range(a.utts):
        row = []
        while len(row) < 1000:
            row += [int(rng.integers(0, 40))] * int(rng.integers(3, 12))
        labels.append(row[:1000])
    for k in range(50):
        src, dst = k % a.utts, (k * 7 + 3) % a.utts
        n = int(rng.integers(50, 151))
        o, at = int(rng.integers(0, 1000 - n)), int(rng.integers(0, 1000 - n))
        if dst != src:
            utts[dst][at:at + n] = utts[src][o:o + n] + 0.05 * rng.standard_normal((n, a.dim)).astype(np.float32)
            labels[dst][at:at + n] = labels[src][o:o + n]
    for i, u in enumerate(utts):
        np.save(os.path.join(feat, f"utt{i}.npy"), u)
    path = os.path.join(root, "labels.txt")
    with open(path, "w") as f:
        for i, row in enumerate(labels):
            f.write(f"utt{i} " + " ".join(str(x) for x in row) + "\n")
    return feat, path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=360)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch_rows", type=int, default=2)
    ap.add_argument("--torch_cols", type=int, default=32)
    ap.add_argument("--numpy_pairs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--probe_lib", type=str, default=os.path.join(ROOT, "bench_out", "liblalign_dp_only.so"))
    ap.add_argument("--build_probe_only", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "term_discovery_bench.json"))
    a = ap.parse_args()
    deps = [os.path.join(lib_build.CSRC, name) for name in ("lalign.hip", "dist_tile.h", "dtw_strip.h")]
    if not os.path.exists(a.probe_lib) or os.path.getmtime(a.probe_lib) < max(os.path.getmtime(p) for p in deps):
        build_probe(a.probe_lib)
    if a.build_probe_only:
        print(a.probe_lib)
        return
    probe = ctypes.CDLL(a.probe_lib)
    for name in ("cpc_local_align_scratch_bytes", "cpc_local_align"):
        getattr(probe, name).restype, getattr(probe, name).argtypes = _lib.SIGNATURES[name]

    dev = torch.device("cuda:0")
    res = {"workload": {"utterances": a.utts, "dim": a.dim, "frames": "300..1500", "seed": a.seed, "params": PARAMS,
                        "probe_params": PROBE_PARAMS}, "fma_rate_per_s": FMA_RATE}
    data = {dist: synthetic(a, dist, dev) for dist in PARAMS}
    lens = data["cosine"][3]
    plan = Plan(lens, tdisc.plan_pairs(np.arange(a.utts), lens), dev)
    res["pairs"], res["segments"], res["cells"] = len(plan.pair_b), len(plan.seg_a), plan.cells
    res["frames_total"] = int(lens.sum())
    res["distance_fma"] = plan.cells * a.dim
    res["floor_distance_s"] = plan.cells * a.dim / FMA_RATE

    # ---- the two kernels on one work list: alternating rounds ----
    arms = [(kernel, dist) for dist in PARAMS for kernel in ("local_align", "sdtw")]

    def run(kernel, dist):
        f, off, ld = data[dist][:3]
        if kernel == "sdtw":
            return plan.sdtw(f, off, ld, td.distance_code(dist))
        return plan.lalign(f, off, ld, td.distance_code(dist), *PARAMS[dist])

    outs = {arm: run(*arm) for arm in arms}                        # warm-up of all
    torch.cuda.synchronize()
    times = {arm: [] for arm in arms}
    for _round in range(a.rounds):
        for arm in arms:
            (score, span), s = event_time(lambda: run(*arm))
            times[arm].append(s)
            assert torch.equal(score, outs[arm][0]) and torch.equal(span, outs[arm][1])              # two launches, the same bits
    for dist in PARAMS:
        f, off, ld = data[dist][:3]
        dp_only = probe_run(probe, plan, f, off, ld, td.distance_code(dist))
        res[dist] = {"theta": PARAMS[dist][0], "gamma": PARAMS[dist][1]}
        for kernel in ("local_align", "sdtw"):
            t = times[(kernel, dist)]
            res[dist][kernel] = {"kernel_s": [round(x, 5) for x in t], "kernel_best_s": min(t), "kernel_spread": (max(t) - min(t)) / min(t),
                                 "cells_per_s": plan.cells / min(t), "distance_tflops": 2 * plan.cells * a.dim / min(t) / 1e12,
                                 "share_of_distance_floor": res["floor_distance_s"] / min(t)}
        best = res[dist]["local_align"]["kernel_best_s"]
        score = outs[("local_align", dist)][0]
        span = outs[("local_align", dist)][1]
        res[dist].update({"local_align_over_sdtw": best / res[dist]["sdtw"]["kernel_best_s"],
                          "dp_only_s": [round(x, 5) for x in dp_only], "dp_only_best_s": min(dp_only),
                          "dp_only_share_of_kernel": min(dp_only) / best, "dp_only_cells_per_s": plan.cells / min(dp_only),
                          "pairs_with_a_match": int((score > 0).sum()), "mean_path_cells": float(span[:, 4].clamp(min=0).float().mean())})

    # ---- plain torch on a subset ----
    order = np.argsort(lens, kind="stable")
    sub_rows = [int(x) for x in order[:a.torch_rows]]
    sub_cols = [int(x) for x in order[a.torch_rows:a.torch_rows + a.torch_cols]]
    sub = Plan(lens, td.plan_segments(sub_rows, sub_cols, lens), dev, rows=sub_rows)
    for dist in PARAMS:
        f, off, ld = data[dist][:3]
        offs = off.cpu().numpy()
        theta, gamma = PARAMS[dist]
        sub.lalign(f, off, ld, td.distance_code(dist), theta, gamma)
        torch.cuda.synchronize()
        (k_score, k_span), k_s = event_time(lambda: sub.lalign(f, off, ld, td.distance_code(dist), theta, gamma))
        cols = ([int(offs[c]) for c in sub_cols], [int(lens[c]) for c in sub_cols])
        torch_local_align(f, int(offs[sub_rows[0]]), 8, cols[0][:2], cols[1][:2], dist, theta, gamma)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_out = [torch_local_align(f, int(offs[r]), int(lens[r]), cols[0], cols[1], dist, theta, gamma) for r in sub_rows]
        torch.cuda.synchronize()
        t_s = time.perf_counter() - t0
        t_score, t_span = torch.cat([o[0] for o in t_out]), torch.cat([o[1] for o in t_out])
        res[dist]["torch_subset"] = {"pairs": len(sub.pair_b), "cells": sub.cells,
                                     "torch_s": t_s, "kernel_s": k_s, "ratio": t_s / k_s,
                                     "max_score_diff": float((t_score - k_score).abs().max()),
                                     "spans_equal": int((t_span == k_span).all(dim=1).sum())}

    # ---- numpy on the host, copy included ----
    for dist in PARAMS:
        f, off, ld = data[dist][:3]
        offs = off.cpu().numpy()
        theta, gamma = PARAMS[dist]
        pairs = [(int(order[2 * k]), int(order[2 * k + 1])) for k in range(a.numpy_pairs)]
        one = Plan(lens, td.plan_segments([p[0] for p in pairs], [[p[1]] for p in pairs], lens), dev, rows=[p[0] for p in pairs])
        one.lalign(f, off, ld, td.distance_code(dist), theta, gamma)
        torch.cuda.synchronize()
        (k_score, k_span), k_s = event_time(lambda: one.lalign(f, off, ld, td.distance_code(dist), theta, gamma))
        t0 = time.perf_counter()
        want = []
        for r, c in pairs:
            rf = f[offs[r]:offs[r] + lens[r]].cpu().numpy()
            cf = f[offs[c]:offs[c] + lens[c]].cpu().numpy()
            want.append(L.local_align(L.frame_distances(rf, cf, dist), np.float32(theta), np.float32(gamma)))
        n_s = time.perf_counter() - t0
        k_score, k_span = k_score.cpu().numpy(), k_span.cpu().numpy()
        res[dist]["numpy_host"] = {"pairs": len(pairs), "cells": one.cells, "numpy_s": n_s,
                                   "kernel_s": k_s, "ratio": n_s / k_s,
                                   "max_score_rel_diff": max(abs(float(k_score[i]) - w[0]) / max(w[0], 1e-30) for i, w in enumerate(want)),
                                   "spans_equal": sum(tuple(k_span[i]) == w[1] for i, w in enumerate(want)),
                                   "clear": sum(bool(w[2]) for w in want)}
    del data
    torch.cuda.empty_cache()

    # ---- the tool on a synthetic hour ----
    with tempfile.TemporaryDirectory(prefix="term_discovery_bench_") as tmp:
        t0 = time.perf_counter()
        feat, label_path = synthetic_hour(a, tmp)
        made = time.perf_counter() - t0
        out_dir = os.path.join(tmp, "out")
        t0 = time.perf_counter()
        r = tool.main(["from_pre_computed", feat, "--file_extension", ".npy", "--threshold", "q1", "--out", out_dir, "--pathPhone",
                       label_path])
        wall = time.perf_counter() - t0
        log = r["log"]
        res["tool_synthetic_hour"] = {"utterances": log["utterances"], "frames": log["frames"], "pairs": log["pairs"],
                                      "cells": log["cells"], "theta": log["theta"], "gamma": log["gamma"],
                                      "distance_percentiles": log["distance_percentiles"], "seconds": log["seconds"], "wall_s": wall,
                                      "make_files_s": made, "matches_written": log["matches_written"], "ned": r["scores"]["ned"],
                                      "coverage": r["scores"]["coverage"]}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
