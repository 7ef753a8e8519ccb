#!/usr/bin/env python3
"""Query-by-example term detection on one MI355X (cpc2_amd/term_detection.py, csrc/sdtw.hip): the subsequence-DTW kernel on a
seeded synthetic search, against a plain-torch restatement on the device, the numpy statement on the host and two floors.

Workload: --queries (200) queries of 50..150 frames against --docs (2 000) documents of 300..1 500 frames, D = 256 Gaussian
frames (rows normalised for the cosine distance), every query against every document, both distances.

  kernel       device events around subsequence_dtw's kernel call (run_segments), the two distances in alternating rounds after
               a warm-up of both; every round's time is listed, with the smallest and the spread (max - min) / min
  torch        the same definition in plain torch on the device, on a subset (--torch_queries x --torch_docs): one matmul + acos
               (or cdist) for the distances of a query against the padded documents, and the DP by anti-diagonals over a batch
               of documents; wall time behind a synchronise, against the kernel on the same subset
  numpy        the float64 statement of tests/sdtw_oracle.py on the host on --numpy_pairs pairs, the copy of their frames from
               the device included; its scores and spans are compared with the kernel's
  floors       (a) the distance multiply-adds (cells x D) at the unpacked f32 FMA rate of DESIGN.md section 11, 78.6 TFLOP/s;
               (b) the DP alone: the kernel built with the distance tile skipped (CPC_SDTW_SKIP_DISTANCES, a probe build of
               sdtw.hip made by this tool into --probe_lib; stand-in distances), on the same work list, and the time per
               anti-diagonal step per resident DP wave that follows from it
  tool         python -m cpc2_amd.eval.term_detection from_pre_computed on a synthetic hour (--hour_docs documents of 8 s at
               10 ms frames, 50 queries cut from them): its wall time by stage, from term_detection_log.json

Prints one JSON line and writes it to --out (default profiles/term_detection_bench.json).
    python tools/term_detection_bench.py [--build_probe_only]
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
from cpc2_amd.eval import term_detection as tool  # noqa: E402
from tests import sdtw_oracle as S  # noqa: E402

FMA_RATE = 78.6e12 / 2             # unpacked f32 FMAs per second (78.6 TFLOP/s)
RESIDENT = 256 * 4                 # workgroups resident at once: 256 CUs x 4 (34 KB of LDS each)


def build_probe(path):
    """sdtw.hip with the distance tile skipped, as a library of its own (same entry points)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        stub = os.path.join(tmp, "stub.cpp")
        with open(stub, "w") as f:
            f.write("namespace cpc { void set_error(const char *, ...) {} }\n")
        cmd = [lib_build.HIPCC] + lib_build.FLAGS + lib_build.DEVICE_FLAGS + ["-DCPC_SDTW_SKIP_DISTANCES", "-shared", "-x", "hip",
               os.path.join(lib_build.CSRC, "sdtw.hip"), stub, "-o", path]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        noise = [ln for ln in res.stdout.splitlines() if ln.strip() and "is not a recognized feature for this target" not in ln]
        if res.returncode != 0:
            raise RuntimeError("probe build failed:\n" + "\n".join(noise))
    return path


def synthetic(a, distance, dev):
    """(frames, item_off, item_len, lens_host, query items, document items): documents first."""
    rng = np.random.default_rng(a.seed)
    doc_lens = rng.integers(300, 1501, a.docs)
    q_lens = rng.integers(50, 151, a.queries)
    lens = np.concatenate([doc_lens, q_lens])
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    frames = torch.randn(int(lens.sum()), a.dim, device=dev, generator=gen)
    if distance == "cosine":
        frames /= frames.norm(dim=1, keepdim=True)
    off = np.concatenate([[0], np.cumsum(lens[:-1])])
    return (frames, torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), lens,
            np.arange(a.docs, a.docs + a.queries), np.arange(a.docs))


class Plan:
    """A work list on the device and what it counts."""

    def __init__(self, lens, queries, docs, dev):
        self.seg_q, self.seg_start, self.pair_doc, self.pair_q = td.plan_segments(queries, docs, lens)
        q_len = lens[np.asarray(queries)[self.pair_q]]
        d_len = lens[self.pair_doc]
        self.cells = int((q_len * d_len).sum())
        strips = -(-q_len // 64)
        tiles = -(-d_len // 64)
        # anti-diagonal steps of the DP wave: per strip and column tile R + C - 1
        self.steps = int((tiles * q_len + strips * d_len - strips * tiles).sum())
        self.max_q, self.max_d = int(q_len.max()), int(d_len.max())
        self.dev_lists = [torch.from_numpy(x).to(dev) for x in (self.seg_q, self.seg_start, self.pair_doc)]

    def run(self, frames, off, lens_d, code):
        return td.run_segments(frames, off, lens_d, *self.dev_lists, self.max_q, self.max_d, code)


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
    nbytes = lib.cpc_sdtw_scratch_bytes(len(plan.seg_q), plan.max_q, plan.max_d)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    score = torch.empty(len(plan.pair_doc), dtype=torch.float32, device=dev)
    span = torch.empty(len(plan.pair_doc), 3, dtype=torch.int32, device=dev)

    def call():
        status = lib.cpc_sdtw(_lib.ptr(frames), frames.size(1), _lib.ptr(off), _lib.ptr(lens_d), int(lens_d.numel()),
                              *[_lib.ptr(x) for x in plan.dev_lists], len(plan.seg_q), plan.max_q, plan.max_d, code, _lib.ptr(score),
                              _lib.ptr(span), _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev))
        if status != 0:
            raise RuntimeError(f"probe cpc_sdtw failed ({status})")
    call()
    torch.cuda.synchronize()
    return [event_time(call)[1] for _ in range(3)]


def torch_sdtw(frames, q_off, q_len, d_offs, d_lens, distance):
    """The definition in plain torch for one query against a batch of documents: (score [B], start, end, length).  Distances by
    one matmul + acos (cosine) or cdist; DP by anti-diagonals, a cell per (document, query row)."""
    dev = frames.device
    B, n, M = len(d_offs), int(q_len), int(max(d_lens))
    q = frames[q_off:q_off + n]
    x = torch.zeros(B, M, frames.size(1), device=dev)
    for b, (o, m) in enumerate(zip(d_offs, d_lens)):
        x[b, :m] = frames[o:o + m]
    if distance == "cosine":
        d = torch.acos(torch.clamp(torch.matmul(x, q.t()), -1, 1)).transpose(1, 2) / np.pi            # [B, n, M]
    else:
        d = torch.cdist(q.unsqueeze(0).expand(B, n, -1), x)
    T = n + M - 1
    rows = torch.arange(n, device=dev)
    skew = torch.full((B, n, T), float("inf"), device=dev)                                           # skew[b, i, t] = d[b, i, t - i]
    skew[:, rows.view(-1, 1), rows.view(-1, 1) + torch.arange(M, device=dev).view(1, -1)] = d
    inf = torch.full((B, n), float("inf"), device=dev)
    zero = torch.zeros(B, n, dtype=torch.long, device=dev)
    p1c, p1l, p1s, p2c, p2l, p2s = inf, zero, zero, inf, zero, zero
    last_v = torch.full((B, M), float("inf"), device=dev)
    last_l = torch.zeros(B, M, dtype=torch.long, device=dev)
    last_s = torch.zeros(B, M, dtype=torch.long, device=dev)

    def down(t, fill):                                         # value of row i - 1 at row i
        return torch.cat([fill[:, :1], t[:, :-1]], dim=1)

    for t in range(T):
        dc = skew[:, :, t]
        up_c, up_l, up_s = down(p1c, inf), down(p1l, zero), down(p1s, zero)
        dg_c, dg_l, dg_s = down(p2c, inf), down(p2l, zero), down(p2s, zero)
        use_dg = (dg_c <= p1c) & (dg_c <= up_c)
        use_lf = ~use_dg & (p1c <= up_c)
        pc = torch.where(use_dg, dg_c, torch.where(use_lf, p1c, up_c))
        pl = torch.where(use_dg, dg_l, torch.where(use_lf, p1l, up_l))
        ps = torch.where(use_dg, dg_s, torch.where(use_lf, p1s, up_s))
        nc, nl, ns = dc + pc, pl + 1, ps
        nc[:, 0], nl[:, 0], ns[:, 0] = dc[:, 0], 1, t                                                 # row 0: a free start at column t
        p2c, p2l, p2s, p1c, p1l, p1s = p1c, p1l, p1s, nc, nl, ns
        j = t - (n - 1)
        if 0 <= j < M:
            last_v[:, j] = nc[:, n - 1] / nl[:, n - 1]
            last_l[:, j], last_s[:, j] = nl[:, n - 1], ns[:, n - 1]
    valid = torch.arange(M, device=dev).view(1, -1) < torch.tensor(d_lens, device=dev).view(-1, 1)
    last_v = torch.where(valid, last_v, torch.full_like(last_v, float("inf")))
    score = last_v.min(dim=1)[0]
    end = (last_v == score.view(-1, 1)).to(torch.int64).argmax(dim=1)                                # the first column among equals
    pick = end.view(-1, 1)
    return score, last_s.gather(1, pick).view(-1), end, last_l.gather(1, pick).view(-1)


def synthetic_hour(a, root):
    """--hour_docs documents of 800 frames as .npy, 50 queries cut from them (a noisy copy of each planted in another
    document): (feature dir, Q.txt, R.txt)."""
    rng = np.random.default_rng(a.seed + 1)
    feat = os.path.join(root, "features")
    os.makedirs(feat)
    docs = [rng.standard_normal((800, a.dim)).astype(np.float32) for _ in range(a.hour_docs)]
    q_lines, r_lines = [], []
    for k in range(50):
        src, dst = k % a.hour_docs, (k * 7 + 3) % a.hour_docs
        n = int(rng.integers(50, 151))
        o = int(rng.integers(0, 800 - n))
        at = int(rng.integers(0, 800 - n))
        if dst != src:
            docs[dst][at:at + n] = docs[src][o:o + n] + 0.05 * rng.standard_normal((n, a.dim)).astype(np.float32)
            r_lines.append(f"q{k} doc{dst} {at / 100:.2f} {(at + n) / 100:.2f}")
        q_lines.append(f"q{k} doc{src} {o / 100:.3f} {(o + n + 0.7) / 100:.3f}")
    for i, d in enumerate(docs):
        np.save(os.path.join(feat, f"doc{i}.npy"), d)
    q_path, r_path = os.path.join(root, "Q.txt"), os.path.join(root, "R.txt")
    with open(q_path, "w") as f:
        f.write("\n".join(q_lines) + "\n")
    with open(r_path, "w") as f:
        f.write("\n".join(r_lines) + "\n")
    return feat, q_path, r_path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--docs", type=int, default=2000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch_queries", type=int, default=4)
    ap.add_argument("--torch_docs", type=int, default=64)
    ap.add_argument("--numpy_pairs", type=int, default=4)
    ap.add_argument("--hour_docs", type=int, default=450)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--probe_lib", type=str, default=os.path.join(ROOT, "bench_out", "libsdtw_dp_only.so"))
    ap.add_argument("--build_probe_only", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "term_detection_bench.json"))
    a = ap.parse_args()
    deps = [os.path.join(lib_build.CSRC, name) for name in ("sdtw.hip", "dist_tile.h", "dtw_strip.h")]
    if not os.path.exists(a.probe_lib) or os.path.getmtime(a.probe_lib) < max(os.path.getmtime(p) for p in deps):
        build_probe(a.probe_lib)
    if a.build_probe_only:
        print(a.probe_lib)
        return
    probe = ctypes.CDLL(a.probe_lib)
    for name in ("cpc_sdtw_scratch_bytes", "cpc_sdtw"):
        getattr(probe, name).restype, getattr(probe, name).argtypes = _lib.SIGNATURES[name]

    dev = torch.device("cuda:0")
    res = {"workload": {"queries": a.queries, "docs": a.docs, "dim": a.dim, "query_frames": "50..150", "doc_frames": "300..1500",
                        "seed": a.seed}, "fma_rate_per_s": FMA_RATE, "resident_workgroups": RESIDENT}
    data = {dist: synthetic(a, dist, dev) for dist in ("cosine", "euclidian")}
    lens, queries, docs = data["cosine"][3], data["cosine"][4], data["cosine"][5]
    plan = Plan(lens, queries, docs, dev)
    res["pairs"], res["segments"], res["cells"], res["dp_steps"] = len(plan.pair_doc), len(plan.seg_q), plan.cells, plan.steps
    res["distance_fma"] = plan.cells * a.dim
    res["floor_distance_s"] = plan.cells * a.dim / FMA_RATE

    # ---- kernel: alternating rounds ----
    outs = {}
    for dist in data:                                              # warm-up of both
        f, off, ld = data[dist][:3]
        outs[dist] = plan.run(f, off, ld, td.distance_code(dist))
    torch.cuda.synchronize()
    times = {dist: [] for dist in data}
    for _round in range(a.rounds):
        for dist in data:
            f, off, ld = data[dist][:3]
            (score, span), s = event_time(lambda: plan.run(f, off, ld, td.distance_code(dist)))
            times[dist].append(s)
            assert torch.equal(score, outs[dist][0]) and torch.equal(span, outs[dist][1])          # two launches, the same bits
    for dist in data:
        t = times[dist]
        f, off, ld = data[dist][:3]
        dp_only = probe_run(probe, plan, f, off, ld, td.distance_code(dist))
        res[dist] = {"kernel_s": [round(x, 5) for x in t], "kernel_best_s": min(t), "kernel_spread": (max(t) - min(t)) / min(t),
                     "cells_per_s": plan.cells / min(t), "distance_tflops": 2 * plan.cells * a.dim / min(t) / 1e12,
                     "share_of_distance_floor": res["floor_distance_s"] / min(t),
                     "dp_only_s": [round(x, 5) for x in dp_only], "dp_only_best_s": min(dp_only),
                     "dp_only_share_of_kernel": min(dp_only) / min(t),
                     "dp_step_ns_per_resident_wave": min(dp_only) * min(RESIDENT, len(plan.seg_q)) / plan.steps * 1e9,
                     "bound_by": "distances" if min(dp_only) < 0.5 * min(t) else "dp"}

    # ---- plain torch on a subset ----
    sub_q = queries[:a.torch_queries]
    sub_d = docs[:a.torch_docs]
    sub = Plan(lens, sub_q, sub_d, dev)
    for dist in data:
        f, off, ld = data[dist][:3]
        offs = off.cpu().numpy()
        sub.run(f, off, ld, td.distance_code(dist))
        torch.cuda.synchronize()
        (k_score, k_span), k_s = event_time(lambda: sub.run(f, off, ld, td.distance_code(dist)))

        def run_torch():
            return [torch_sdtw(f, int(offs[q]), int(lens[q]), [int(offs[d]) for d in sub_d], [int(lens[d]) for d in sub_d], dist)
                    for q in sub_q]
        torch_sdtw(f, int(offs[sub_q[0]]), int(lens[sub_q[0]]), [int(offs[d]) for d in sub_d[:2]], [int(lens[d]) for d in sub_d[:2]], dist)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_out = run_torch()
        torch.cuda.synchronize()
        t_s = time.perf_counter() - t0
        t_score = torch.cat([o[0] for o in t_out])
        t_span = torch.stack([torch.cat([o[k] for o in t_out]) for k in (1, 2, 3)], dim=1).to(torch.int32)
        res[dist]["torch_subset"] = {"pairs": len(sub.pair_doc), "cells": sub.cells, "torch_s": t_s, "kernel_s": k_s, "ratio": t_s / k_s,
                                     "max_score_diff": float((t_score - k_score).abs().max()),
                                     "spans_equal": int((t_span == k_span).all(dim=1).sum())}

    # ---- numpy on the host, copy included ----
    for dist in data:
        f, off, ld = data[dist][:3]
        offs = off.cpu().numpy()
        pairs = [(int(queries[k]), int(docs[(7 * k) % len(docs)])) for k in range(a.numpy_pairs)]
        one = Plan(lens, [p[0] for p in pairs], [[p[1]] for p in pairs], dev)
        one.run(f, off, ld, td.distance_code(dist))
        torch.cuda.synchronize()
        (k_score, k_span), k_s = event_time(lambda: one.run(f, off, ld, td.distance_code(dist)))
        t0 = time.perf_counter()
        want = []
        for q, d in pairs:
            qf = f[offs[q]:offs[q] + lens[q]].cpu().numpy()
            df = f[offs[d]:offs[d] + lens[d]].cpu().numpy()
            want.append(S.sdtw(S.frame_distances(qf, df, dist)))
        n_s = time.perf_counter() - t0
        k_score, k_span = k_score.cpu().numpy(), k_span.cpu().numpy()
        res[dist]["numpy_host"] = {"pairs": len(pairs), "cells": one.cells, "numpy_s": n_s, "kernel_s": k_s, "ratio": n_s / k_s,
                                   "max_score_diff": max(abs(float(k_score[i]) - w[0]) for i, w in enumerate(want)),
                                   "spans_equal": sum(tuple(k_span[i]) == w[1:4] for i, w in enumerate(want)),
                                   "clear": sum(bool(w[4]) for w in want)}
    del data
    torch.cuda.empty_cache()

    # ---- the tool on a synthetic hour ----
    with tempfile.TemporaryDirectory(prefix="term_detection_bench_") as tmp:
        t0 = time.perf_counter()
        feat, q_path, r_path = synthetic_hour(a, tmp)
        made = time.perf_counter() - t0
        out_dir = os.path.join(tmp, "out")
        t0 = time.perf_counter()
        r = tool.main(["from_pre_computed", feat, "--file_extension", ".npy", "--queries", q_path, "--relevance", r_path, "--out", out_dir])
        wall = time.perf_counter() - t0
        log = json.load(open(os.path.join(out_dir, "term_detection_log.json")))
        res["tool_synthetic_hour"] = {"documents": log["documents"], "queries": log["queries"], "frames": log["frames"],
                                      "pairs": log["pairs"], "cells": log["cells"], "seconds": log["seconds"], "wall_s": wall,
                                      "make_files_s": made, "map": r["scores"]["map"], "span_iou_at_0.5": r["scores"]["span_iou_at_0.5"]}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
