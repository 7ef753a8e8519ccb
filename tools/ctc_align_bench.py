#!/usr/bin/env python3
"""Timings of CTC forced alignment on one MI355X ("CTC forced alignment").  Prints one JSON object and writes it to
--out.  Times only: nothing here is a promise.

  1. cpc_ctc_align and cpc_ctc_align_segments on b = 8 and 64 sequences of T = 250 / 1000 / 4096 frames with L = T / 4 labels
     and k = 41 classes (random logits, every input length = T): device events around one launch each, the configurations
     taken in turn for --rounds rounds; median, minimum and maximum per configuration.
  2. The same batches through (a) tests/ctc_align_oracle.py, the numpy float64 statement on this host's CPU, INCLUDING the copy
     of the logits to the host (wall seconds, once), and (b) a plain-torch restatement on the device with one set of launches
     per frame, forward and backtrace (device events, --torch-rounds rounds).  Both are checked to return the kernel's paths.
  3. `common_voices_eval align` by stage (audio, model, head, alignment, writing; the device is synchronised behind each stage)
     on a synthetic hour: 240 noise utterances of 10 to 20 s through the recorded CPC checkpoint of tests/golden and a seeded
     head, a fifth as many labels as head frames.

    python tools/ctc_align_bench.py [--rounds 15] [--torch-rounds 3] [--hours 1.0] [--out profiles/ctc_align_bench.json]
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
import ctc_align_oracle  # noqa: E402
from cpc2_amd import _lib  # noqa: E402
from cpc2_amd.eval import common_voices_eval as cv  # noqa: E402
from cpc2_amd.feature_loader import loadModel  # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 41


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
    """One batch and its output buffers; align() and segments() are one launch each."""

    def __init__(self, b, t, seed=0):
        g = torch.Generator().manual_seed(seed + 1000 * b + t)
        self.b, self.t, self.max_l = b, t, t // 4
        self.logits = (torch.randn(b, t, K, generator=g) * 3).to(DEV)
        self.targets = torch.randint(0, K - 1, (b, self.max_l), generator=g).to(DEV)
        self.in_len = torch.full((b,), t, dtype=torch.int64, device=DEV)
        self.tgt_len = torch.full((b,), self.max_l, dtype=torch.int64, device=DEV)
        self.path = torch.empty(b, t, dtype=torch.int32, device=DEV)
        self.score = torch.empty(b, 2, dtype=torch.float64, device=DEV)
        self.status = torch.empty(b, dtype=torch.int32, device=DEV)
        self.ties = torch.empty(b, dtype=torch.int32, device=DEV)
        self.lse = torch.empty(b, t, dtype=torch.float64, device=DEV)
        self.first = torch.empty(b, self.max_l, dtype=torch.int32, device=DEV)
        self.last = torch.empty(b, self.max_l, dtype=torch.int32, device=DEV)
        self.conf = torch.empty(b, self.max_l, dtype=torch.float32, device=DEV)
        self.lib = _lib.load()
        self.nbytes = self.lib.cpc_ctc_align_scratch_bytes(b, t, self.max_l)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=DEV)

    def align(self):
        p = _lib.ptr
        _lib.check(self.lib.cpc_ctc_align(p(self.logits), self.b, self.t, K, p(self.in_len), p(self.targets), self.max_l, p(self.tgt_len),
                                          p(self.path), p(self.score), p(self.status), p(self.ties), p(self.lse), p(self.scratch),
                                          self.nbytes, _lib.stream_ptr(DEV)), "ctc_align")

    def segments(self):
        p = _lib.ptr
        _lib.check(self.lib.cpc_ctc_align_segments(p(self.logits), self.b, self.t, K, p(self.targets), self.max_l, p(self.tgt_len),
                                                   p(self.path), p(self.status), p(self.lse), p(self.first), p(self.last), p(self.conf),
                                                   _lib.stream_ptr(DEV)), "ctc_align_segments")


def torch_align(logits, targets):
    """The definition in plain torch on the device, every length full: one set of launches per frame forward, one per frame back.
    Returns (path int64 [b, T], score float64 [b])."""
    b, t, k = logits.shape
    n_lab = targets.shape[1]
    n_states = 2 * n_lab + 1
    neg = float("-inf")
    sym = torch.full((b, n_states), k - 1, dtype=torch.int64, device=logits.device)
    sym[:, 1::2] = targets
    allow2 = torch.zeros(b, n_states, dtype=torch.bool, device=logits.device)
    allow2[:, 3::2] = sym[:, 3::2] != sym[:, 1:-2:2]
    emit = logits.double().gather(2, sym.unsqueeze(1).expand(b, t, n_states))          # (one gather for all frames)
    v = torch.full((b, n_states), neg, dtype=torch.float64, device=logits.device)
    v[:, :2] = emit[:, 0, :2]
    moves = torch.zeros(t, b, n_states, dtype=torch.uint8, device=logits.device)
    pad = torch.full((b, 2), neg, dtype=torch.float64, device=logits.device)
    for f in range(1, t):
        c1 = torch.cat([pad[:, :1], v[:, :-1]], 1)
        c2 = torch.where(allow2, torch.cat([pad, v[:, :-2]], 1), pad[:, :1])
        best, mv = torch.stack([v, c1, c2]).max(0)               # (which of equal maxima wins is torch's business: compared when no tie was met)
        v = best + emit[:, f]
        moves[f] = mv
    end = torch.where(v[:, -2] > v[:, -1], n_states - 2, n_states - 1)
    score = v.gather(1, end.unsqueeze(1))[:, 0]
    path = torch.empty(b, t, dtype=torch.int64, device=logits.device)
    s = end
    for f in range(t - 1, -1, -1):
        path[:, f] = s
        s = s - moves[f].gather(1, s.unsqueeze(1))[:, 0].long()
    return path, score


def kernels(rounds, torch_rounds):
    out = {"classes": K, "labels": "T / 4", "shapes": {}}
    for b in (8, 64):
        for t in (250, 1000, 4096):
            case = Case(b, t)
            arms = {"align": case.align, "segments": case.segments}
            for fn in arms.values():
                fn()
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(rounds):
                for k, fn in arms.items():
                    ms[k].append(once(fn)[0])
            rec = {k: stats(v) for k, v in ms.items()}
            rec["scratch_MB"] = case.nbytes / 2 ** 20
            rec["aligned"] = int((case.status == 0).sum())
            rec["tied"] = int(case.ties.sum())
            # (a) the float64 statement on the host, the copy of the logits included
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = case.logits.cpu().numpy()
            refs = ctc_align_oracle.align_batch(host, [t] * b, case.targets.cpu().numpy(), [case.max_l] * b)
            rec["host_numpy_f64_s"] = time.perf_counter() - t0
            rec["host_equal"] = bool(all(np.array_equal(r["path"], p) for r, p in zip(refs, case.path.cpu().numpy())))
            # (b) plain torch on the device
            torch_align(case.logits[:, :8], case.targets[:, :2])           # (code objects)
            tm = [once(lambda: torch_align(case.logits, case.targets)) for _ in range(torch_rounds)]
            rec["plain_torch"] = stats([m for m, _ in tm])
            rec["plain_torch_equal"] = bool(torch.equal(tm[-1][1][0].int(), case.path)) if rec["tied"] == 0 else None
            out["shapes"][f"b{b}_T{t}"] = rec
            print(f"b={b} T={t}: {json.dumps(rec)}", file=sys.stderr, flush=True)
            del case
            torch.cuda.empty_cache()
    return out


class SyntheticUtterances(cv.SingleSequenceDataset):
    """Noise utterances of 10 to 20 s made on the device instead of read from files."""

    def __init__(self, hours, n_phones, seed=0):
        self.hours, self.n_phones, self.seed = hours, n_phones, seed
        super().__init__(None, [], {}, random_offset_amplitude=0, device=DEV)

    def loadSeqs(self):
        rng = np.random.default_rng(self.seed)
        sizes = []
        while sum(sizes) < self.hours * 3600 * 16000:
            sizes.append(int(rng.integers(160000, 320001)))
        labels = [rng.integers(0, self.n_phones, max(size // 160 // 4 // 5, 1)) for size in sizes]
        self.names = [f"synthetic-{i:04d}" for i in range(len(sizes))]
        self.seqOffset = [0] + [int(v) for v in np.cumsum(sizes)]
        self.phoneOffsets = [0] + [int(v) for v in np.cumsum([len(y) for y in labels])]
        self.maxSize, self.maxSizePhone = max(sizes), max(len(y) for y in labels)
        g = torch.Generator(device=DEV).manual_seed(self.seed)
        self.data = torch.randn(int(sum(sizes)), generator=g, device=DEV) * 0.1
        self.phoneLabels = torch.from_numpy(np.concatenate(labels)).long()


def tool(hours, batch):
    ckpt = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
    model, hidden, _ = loadModel([ckpt])
    model.to(DEV).eval()
    model.optimize = False
    torch.manual_seed(0)
    crit = cv.CTCphone_criterion(hidden, K - 1).to(DEV)
    with torch.no_grad():
        for p in crit.PhoneCriterionClassifier.parameters():
            p.mul_(8.0)
    t0 = time.perf_counter()
    ds = SyntheticUtterances(hours, K - 1)
    torch.cuda.synchronize()
    out = dict(utterances=len(ds), batch=batch, audio_hours=float(ds.seqOffset[-1]) / 16000 / 3600, synthesis_s=time.perf_counter() - t0)
    for rep in range(2):                               # the second pass is the record (the first loads code objects)
        with tempfile.TemporaryDirectory() as tmp:
            timings = {}
            t0 = time.perf_counter()
            log = cv.alignStep(ds.batches(batch, shuffle=False), ds.names, model, crit, 160, tmp, timings=timings)
            torch.cuda.synchronize()
            out["stages_s"] = timings
            out["total_s"] = time.perf_counter() - t0
            out["aligned"], out["met_a_tie"] = log["aligned"], log["met_a_tie"]
            out["frames_file_MB"] = os.path.getsize(os.path.join(tmp, "alignment_frames.txt")) / 2 ** 20
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernels": kernels(args.rounds, args.torch_rounds),
           "tool": tool(args.hours, args.batch)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
