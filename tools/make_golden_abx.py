#!/usr/bin/env python3
"""Generate tests/golden/g19_abx.npz (+ the item files g19_abx_synth.item, g19_abx_test_db.item) by running the
REFERENCE's ABX evaluation (cpc/eval/eval_ABX.py, cpc/eval/ABX) on the CPU.

Runs only in the build container where /root/reference exists:
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_abx.py

The reference is imported unmodified.  progressbar (a no-op ProgressBar) and torchaudio are stubbed; the Cython DTW
(dtw.pyx) is compiled by pyximport into a temporary directory outside the repository.  Only inputs and outputs are
written.  random.sample is wrapped (by this script) to record every draw the reference makes.
"""
import json
import math
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")


class _ProgressBar:
    def __init__(self, *a, **k):
        pass

    def start(self):
        pass

    def update(self, *a):
        pass

    def finish(self):
        pass


sys.modules["progressbar"] = types.SimpleNamespace(ProgressBar=_ProgressBar)
sys.modules.setdefault("torchaudio", types.ModuleType("torchaudio"))
import pyximport  # noqa: E402

_BUILD = tempfile.mkdtemp(prefix="abx_dtw_build_")
pyximport.install(build_dir=_BUILD, setup_args={"include_dirs": np.get_include()}, language_level=3)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "cpc", "eval"))
import ABX.abx_group_computation as ref_g  # noqa: E402
import ABX.abx_iterators as ref_it  # noqa: E402
import eval_ABX as ref_eval  # noqa: E402

torch.set_num_threads(8)
ARR = {}
DRAWS = []
_sample = random.sample


def _recording_sample(population, k):
    out = _sample(population, k=k)
    DRAWS.append(json.dumps([list(v) if isinstance(v, tuple) else v for v in out]))
    return out


random.sample = _recording_sample


# --------------------------------------------------------------------------- DTW cases
def padded(rng, lengths, D, kind):
    S = max(lengths)
    x = torch.zeros(len(lengths), S, D)
    for i, n in enumerate(lengths):
        if kind == "int":
            v = torch.from_numpy(rng.integers(-2, 3, size=(n, D)).astype(np.float32))
        else:
            v = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32))
        if kind == "cos":
            v[rng.random(n) < 0.15] = 0.0                                 # zero frames
            v = ref_it.normalize_with_singularity(v)[:, :D]              # drop the border: re-added below
        x[i, :n] = v
    return x, torch.tensor(lengths)


def dtw_case(k, rng, l1, l2, D, kind, symmetric):
    if kind == "cos":                                # normalised inputs with the singularity column, as ABX feeds them
        a, sa = padded(rng, l1, D, "raw")
        b, sb = padded(rng, l2, D, "raw")
        for t, s in ((a, sa), (b, sb)):
            for i, n in enumerate(s.tolist()):
                t[i, :n][torch.from_numpy(rng.random(n) < 0.15)] = 0.0
        a = torch.stack([torch.cat([ref_it.normalize_with_singularity(a[i, :n].clone()),
                                    torch.zeros(a.size(1) - n, D + 1)]) for i, n in enumerate(sa.tolist())])
        b = torch.stack([torch.cat([ref_it.normalize_with_singularity(b[i, :n].clone()),
                                    torch.zeros(b.size(1) - n, D + 1)]) for i, n in enumerate(sb.tolist())])
        fn = ref_g.get_cosine_distance_batch
    else:
        a, sa = padded(rng, l1, D, kind)
        b, sb = padded(rng, l2, D, kind)
        fn = ref_g.get_euclidian_distance_batch
    if symmetric:
        b, sb = a, sa
    out = ref_g.get_distance_group_dtw(a, b, sa, sb, ignore_diag=symmetric, symmetric=symmetric, distance_function=fn)
    ARR[f"dtw{k}_a"], ARR[f"dtw{k}_sa"] = a.numpy(), sa.numpy()
    ARR[f"dtw{k}_b"], ARR[f"dtw{k}_sb"] = b.numpy(), sb.numpy()
    ARR[f"dtw{k}_cfg"] = np.array([0 if kind == "cos" else 1, int(symmetric)])
    ARR[f"dtw{k}_out"] = out.numpy()


def dtw_cases():
    rng = np.random.default_rng(1901)
    cases = [([1, 5, 13], [1, 7, 20, 3], 3, "cos", False),
             ([64, 65, 90], [1, 63, 90], 3, "cos", False),
             ([17, 25, 4], [9, 25, 3, 12], 256, "cos", False),
             ([70, 12, 33], None, 24, "cos", True),
             ([1, 20, 90], [2, 64, 41], 24, "euc", False),
             ([9, 14, 22, 5], None, 24, "euc", True),
             ([6, 11, 15], [7, 10, 16], 3, "int", False),
             ([8, 12, 5, 9], None, 3, "int", True)]
    for k, (l1, l2, D, kind, sym) in enumerate(cases):
        dtw_case(k, rng, l1, l2 or l1, D, kind, sym)
    ARR["dtw_n"] = np.array(len(cases))
    # cpc/eval/ABX/unit_tests.py:17-56: two known distances and one known theta
    X = torch.tensor([[[0, 1], [0, 0], [1, 1], [42, 42]], [[0, 2], [0, 1], [1, 1], [-1, 0]],
                      [[0, 0], [0, 1], [0, 0], [21, 211]]], dtype=torch.float)
    X_size = torch.tensor([3, 4, 2])
    Y = torch.tensor([[[0, 1], [1, 2], [0, 0]]], dtype=torch.float)
    Y_size = torch.tensor([3])
    ARR["known_X"], ARR["known_X_size"], ARR["known_Y"], ARR["known_Y_size"] = X.numpy(), X_size.numpy(), Y.numpy(), Y_size.numpy()
    ARR["known_dist"] = ref_g.get_distance_group_dtw(X, Y, X_size, Y_size,
                                                     distance_function=ref_g.get_euclidian_distance_batch).numpy()
    ARR["known_expected"] = np.array([math.sqrt(2) / 2, 3 / 4, (2 + math.sqrt(2)) / 3])
    ARR["known_theta"] = np.array(ref_g.get_theta_group_dtw(X, Y, X, X_size, Y_size, X_size,
                                                            ref_g.get_euclidian_distance_batch, True))


# --------------------------------------------------------------------------- ABX cases
def write_synth_items(path, rng):
    """6 files x ~4 s, 4 speakers, 4 phones, 3 contexts; phones of 30-160 ms at 100 frames / s."""
    lines = ["#file onset offset #phone prev-phone next-phone speaker"]
    phones, contexts, speakers = ["aa", "b", "ih", "s"], [("n", "t"), ("d", "l"), ("m", "k")], ["s1", "s2", "s3", "s4"]
    files = {}
    for f in range(6):
        fid = f"f{f}"
        spk = speakers[f % 4]
        t = 0.05
        frames = 400
        files[fid] = (frames, spk)
        while t < frames / 100 - 0.3:
            dur = float(rng.integers(3, 17)) / 100 + float(rng.integers(0, 10)) / 1000
            ph = phones[int(rng.integers(0, 4))]
            c = contexts[int(rng.integers(0, 3))]
            lines.append(f"{fid} {t:.4f} {t + dur:.4f} {ph} {c[0]} {c[1]} {spk}")
            t += dur + float(rng.integers(0, 5)) / 100
    # an item past the end of its file and an empty one: both skipped
    lines.append(f"f0 4.5000 4.7000 aa n t s1")
    lines.append(f"f1 1.0000 1.0040 b d l s2")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return files, phones, speakers


def synth_features(rng, files, item_path, D, three_d):
    data, _, phone_match, speaker_match = ref_it.load_item_file(item_path)
    feats = {}
    pmean = rng.standard_normal((len(phone_match), D)).astype(np.float32) * 1.0
    soff = rng.standard_normal((len(speaker_match), D)).astype(np.float32) * 0.7
    for fid, (frames, spk) in files.items():
        x = rng.standard_normal((frames, D)).astype(np.float32) * 1.6
        for on, off, _c, p, s in data[fid]:
            i0, i1 = max(0, math.ceil(100 * on - 0.5)), min(frames, math.floor(100 * off - 0.5))
            x[i0:i1] += pmean[p] + soff[s]
        x[rng.random(frames) < 0.04] = 0.0                                   # zero frames
        feats[fid] = torch.from_numpy(x).view(1, frames, D) if three_d else torch.from_numpy(x)
    return feats


def abx_case(tag, feats, item_path, seed, step, max_size_group, max_x_across):
    seq_list = [(fid, fid) for fid in sorted(feats)]

    def fn(path):
        return feats[path].clone()                       # normalize_with_singularity works in place

    for k, v in feats.items():
        ARR[f"{tag}_feat_{k}"] = v.numpy()
    ARR[f"{tag}_cfg"] = np.array([seed, step, max_size_group, max_x_across])
    # per-mode sparse tensors, both modes back to back as ABX() runs them
    DRAWS.clear()
    random.seed(seed)
    ds = ref_it.ABXFeatureLoader(item_path, seq_list, fn, step, True)
    ARR[f"{tag}_features"] = np.array(ds.features, dtype=np.float64)
    ARR[f"{tag}_data"] = ds.data.numpy()
    for mode in ("within", "across"):
        it = ds.get_iterator(mode, max_size_group, max_x_across)
        sp = ref_g.get_abx_scores_dtw_on_group(it, ref_g.get_cosine_distance_batch, it.symmetric)
        ARR[f"{tag}_{mode}_coords"] = sp._indices().numpy().T
        ARR[f"{tag}_{mode}_values"] = sp._values().numpy()
        ARR[f"{tag}_{mode}_board"] = np.array(sp.size())
        ARR[f"{tag}_{mode}_len"] = np.array(len(it))
    ARR[f"{tag}_draws"] = np.array(list(DRAWS))
    random.seed(seed)
    scores = ref_eval.ABX(fn, item_path, seq_list, "cosine", step, ["within", "across"], cuda=False,
                          max_x_across=max_x_across, max_size_group=max_size_group)
    ARR[f"{tag}_scores"] = np.array([scores["within"], scores["across"]])
    print(tag, scores, len(DRAWS), "draws")


def write_test_db_items(path, rng):
    """Phone-like items over the committed LibriSpeech excerpts (tests/golden/test_db), first 5 s of each file."""
    lines = ["#file onset offset #phone prev-phone next-phone speaker"]
    db = os.path.join(OUT, "test_db")
    for dirpath, _d, names in sorted(os.walk(db)):
        for n in sorted(names):
            if not n.endswith(".flac"):
                continue
            stem = n[:-5]
            spk = stem.split("-")[0]
            t = 0.1
            while t < 4.7:
                dur = float(rng.integers(4, 15)) / 100
                ph = "abcde"[int(rng.integers(0, 5))]
                c = [("x", "y"), ("y", "z")][int(rng.integers(0, 2))]
                lines.append(f"{stem} {t:.3f} {t + dur:.3f} {ph} {c[0]} {c[1]} {spk}")
                t += dur + 0.02
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    dtw_cases()
    rng = np.random.default_rng(1902)
    item_path = os.path.join(OUT, "g19_abx_synth.item")
    files, _, _ = write_synth_items(item_path, rng)
    abx_case("abx2d", synth_features(rng, files, item_path, 12, False), item_path, 1234, 100.0, 3, 2)
    abx_case("abx3d", synth_features(rng, files, item_path, 12, True), item_path, 99, 100.0, 3, 2)
    write_test_db_items(os.path.join(OUT, "g19_abx_test_db.item"), np.random.default_rng(1903))
    ARR["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(OUT, "g19_abx.npz"), **ARR)
    print("wrote g19_abx.npz", os.path.getsize(os.path.join(OUT, "g19_abx.npz")), "bytes")


if __name__ == "__main__":
    main()
