#!/usr/bin/env python3
"""Timings of the phone-error-rate path on one MI355X ("Phone error rate").  Prints one JSON object and writes it to
--out.

  1. cpc_ctc_beam_search on 64 windows of [128, 42] peaked probabilities (one class per frame at about 0.9) at nKeep 20 and
     100, all prefixes and best prefix only, and cpc_align_score on the 64 (collapsed labels, best prefix) pairs: device events
     around one call each, the configurations taken in turn for --rounds rounds; median, minimum and maximum per configuration;
  2. tests/per_oracle.py (the float32 numpy statement of the reference's search) on ONE of those windows on this host's CPU;
  3. `python -m cpc2_amd.eval.phone_error_rate` on a probe directory built from tests/golden (the recorded CPC checkpoint, a
     seeded classifier scaled by 40, the two labelled files of tests/golden/test_db): wall time by stage.

    python tools/per_bench.py [--rounds 15] [--out profiles/per_bench.json]
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
import per_oracle  # noqa: E402
from cpc2_amd import criterion as cr  # noqa: E402
from cpc2_amd import feature_loader as fl  # noqa: E402
from cpc2_amd import seq_alignment as sa  # noqa: E402
from cpc2_amd.dataset import parseSeqLabels  # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def peaked(n, T=128, P=42, conf=0.9, seed=0):
    g = torch.Generator().manual_seed(seed)
    path = torch.randint(0, P, (n, T), generator=g)
    logits = torch.randn(n, T, P, generator=g)
    logits.scatter_add_(2, path[..., None], torch.full((n, T, 1), float(np.log(conf / (1 - conf) * (P - 1)))))
    return torch.softmax(logits, 2), path


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), rounds=len(ms))


def kernels(rounds):
    probs, path = peaked(64)
    probs = probs.to(DEV)
    labels, sizes = sa.collapse_padded(path.to(DEV))
    configs = {"search_k20_all": lambda: sa.beam_search_batch(probs, None, 20, 41),
               "search_k20_best": lambda: sa.beam_search_batch(probs, None, 20, 41, best_only=True),
               "search_k100_all": lambda: sa.beam_search_batch(probs, None, 100, 41),
               "search_k100_best": lambda: sa.beam_search_batch(probs, None, 100, 41, best_only=True)}
    best = configs["search_k100_best"]()
    configs["align_64_pairs"] = lambda: sa.align_score_batch(labels, sizes, best[2][:, 0], best[1][:, 0], -1, -1, 0)
    for fn in configs.values():                      # warm-up: buffers, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in configs}
    for _ in range(rounds):
        for k, fn in configs.items():
            ms[k].append(once(fn)[0])
    out = {k: stats(v) for k, v in ms.items()}
    out["windows"], out["frames"], out["classes"] = 64, 128, 42
    out["tied_windows_k100"] = int(best[4].sum())
    out["mean_best_length"] = float(best[1].double().mean())
    window = probs[0].cpu().numpy()
    for k in (20, 100):
        t0 = time.perf_counter()
        ref, tie = per_oracle.beam_search(window, k, 41)
        out[f"oracle_one_window_k{k}_s"] = time.perf_counter() - t0
        got = sa.beam_search(window, k, 41)
        out[f"oracle_equal_k{k}"] = bool(not tie and [(np.float32(s).tobytes(), l) for s, l in ref] ==
                                         [(np.float32(s).tobytes(), l) for s, l in got])
    return out


def tool():
    from cpc2_amd.eval import phone_error_rate as per
    ckpt = os.path.join(GOLDEN, "ref_checkpoint", "checkpoint_7.pt")
    phones = os.path.join(GOLDEN, "phone_labels.txt")
    model, hidden_gar, _ = fl.loadModel([ckpt])
    _, n_phones = parseSeqLabels(phones)
    torch.manual_seed(26)
    crit = cr.CTCPhoneCriterion(hidden_gar, n_phones, False)
    with torch.no_grad():
        for p in crit.parameters():
            p.mul_(40.0)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        val = os.path.join(tmp, "val.txt")
        with open(val, "w") as f:
            f.write("2911-12359-0007\n4051-11218-0044\n")
        with open(os.path.join(tmp, "checkpoint_args.json"), "w") as f:
            json.dump(dict(pathDB=os.path.join(GOLDEN, "test_db"), pathVal=val, load=[ckpt], pathPhone=phones, CTC=True,
                           batchSizeGPU=8, file_extension=".flac", get_encoded=False, size_window=20480), f)
        fl.save_checkpoint(model.state_dict(), crit.state_dict(), {}, model.state_dict(), os.path.join(tmp, "checkpoint_0.pt"))
        for n_keep in (20, 100):
            for _ in range(2):                       # the second run is the record (the first loads code objects)
                per.main([tmp, "--nKeep", str(n_keep), "--out", os.path.join(tmp, "per.json")])
            with open(os.path.join(tmp, "per.json")) as f:
                res = json.load(f)
            out[f"k{n_keep}"] = {k: res[k] for k in ("mean", "std", "windows", "tied_windows", "seconds")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernels": kernels(args.rounds), "tool": tool()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
