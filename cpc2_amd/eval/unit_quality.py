"""How well a unit inventory stands for phones, and what it costs in bits (cpc2_amd/unit_scores.py, csrc/unit_scores.hip;
DESIGN.md section 24).  The reference has no such tool; the command line has the shape of eval_ABX_clustering.

    python -m cpc2_amd.eval.unit_quality --quantized QUANT_DIR/quantized_outputs.txt [--pathPhone LABELS.txt] --out DIR
    python -m cpc2_amd.eval.unit_quality --clustering OUT_DIR/checkpoint_last.pt --path_audio_data AUDIO_DIR
           [--file_extension .flac] [--pathPhone LABELS.txt] --out DIR
    common flags: [--pathSeqs LIST] [--tolerance 2] [--max_length_mismatch 2] [--feature_size 0.01] [--n_units K] [--n_phones P]

--quantized reads the file clustering_quantization writes (`name<TAB>u,u,...`, one unit per frame; a line with `a-b` group tokens
is refused by name).  --clustering rebuilds the feature maker and the centroids as eval_ABX_clustering --clustering does and
assigns every frame with cpc_kmeans_assign; the units never leave the device.  Labels (--pathPhone) are what parseSeqLabels reads:
the label files of linear_separability, or the alignment_frames.txt of `common_voices_eval align`.  --n_units and --n_phones default
to the largest value seen plus one (--clustering: the number of centroids).

An utterance without a label line is listed as skipped; one whose two lengths differ by more than --max_length_mismatch frames is
listed as mismatched and left out; otherwise the first min(frames, labels) frames are compared (the policy of phone_segmentation).
Without --pathPhone only the unit-side numbers are made (entropy, perplexity, bitrates, run length).  Three files are written:
    unit_scores.json     the arguments, the scores (unit_scores.scores), the totals, skipped and mismatched by name
    joint_counts.npy     int64 [n_units, n_phones]
    unit_to_phone.txt    `unit phone count frames purity` per used unit

Refused by name before any audio or feature file is opened: a non-empty --out, both sources or neither, --clustering without
--path_audio_data, --file_extension .mp3, --feature_size <= 0, a negative --tolerance or --max_length_mismatch, --n_units or
--n_phones outside the kernel's limits.  When every utterance was skipped or mismatched the tool raises ValueError.
"""
import argparse
import json
import os
import sys
from os.path import basename, splitext
from pathlib import Path

import numpy as np
import torch

from .. import unit_scores as us
from ..dataset import filterSeqs, findAllSeqs, parseSeqLabels

BATCH_UTTERANCES = 1 << 16        # utterances per call of unit_scores.count (the kernels take 2^20)


def parse_args(argv):
    parser = argparse.ArgumentParser(description="Purity, PNMI and bitrate of quantized units against phone labels. Use either "
                                                 "--quantized pathQuantized or --clustering pathClustering")
    parser.add_argument("--quantized", type=str, default=None, help="The quantized_outputs.txt of clustering_quantization")
    parser.add_argument("--clustering", type=str, default=None, help="The checkpoint of the clustering module")
    parser.add_argument("--path_audio_data", type=str, default=None, help="The audio dataset (--clustering)")
    parser.add_argument("--file_extension", type=str, default=".flac", help=".wav or .flac (.mp3 is refused)")
    parser.add_argument("--pathPhone", type=str, default=None, help="Frame-level phone labels, `name l0 l1 ...` per line")
    parser.add_argument("--pathSeqs", type=str, default=None, help="List of the utterances to score (base names)")
    parser.add_argument("--tolerance", type=int, default=2, help="Boundary matching tolerance in frames (2 = 20 ms)")
    parser.add_argument("--max_length_mismatch", type=int, default=2,
                        help="Largest difference in frames between units and labels of a scored utterance")
    parser.add_argument("--feature_size", type=float, default=0.01, help="Size (in s) of one frame")
    parser.add_argument("--n_units", type=int, default=None, help="Size of the unit inventory (default: largest unit + 1)")
    parser.add_argument("--n_phones", type=int, default=None, help="Number of phone classes (default: largest label + 1)")
    parser.add_argument("--out", type=str, required=True, help="Directory the results are written into (empty or absent)")
    return parser.parse_args(argv)


def check_args(args):
    """The refusals, each naming its flag; nothing has been read yet."""
    if (args.quantized is None) == (args.clustering is None):
        raise ValueError("--quantized / --clustering: give exactly one of the two sources")
    if args.clustering is not None and args.path_audio_data is None:
        raise ValueError("--clustering needs --path_audio_data: the units are made from the audio files")
    if args.file_extension.lower() == ".mp3":
        raise NotImplementedError("--file_extension .mp3: there is no mp3 decoder in this package; convert the files to .wav or .flac")
    if not args.feature_size > 0:
        raise ValueError(f"--feature_size {args.feature_size} must be positive")
    if args.tolerance < 0 or args.max_length_mismatch < 0:
        raise ValueError("--tolerance and --max_length_mismatch must be >= 0")
    if args.n_units is not None and not 1 <= args.n_units <= us.MAX_UNITS:
        raise ValueError(f"--n_units {args.n_units}: the kernel takes 1 .. {us.MAX_UNITS} units")
    if args.n_phones is not None and not 1 <= args.n_phones <= us.MAX_PHONES:
        raise ValueError(f"--n_phones {args.n_phones}: the kernel takes 1 .. {us.MAX_PHONES} phones")
    if args.n_phones is not None and args.pathPhone is None and args.n_phones != 1:
        raise ValueError(f"--n_phones {args.n_phones} without --pathPhone: without labels there is one class")
    if os.path.exists(args.out) and (not os.path.isdir(args.out) or os.listdir(args.out)):
        raise ValueError(f"--out {args.out} exists and is not an empty directory: the tool writes its files there and overwrites "
                         "nothing")
    return args


def read_quantized(path):
    """[(name, int32 array of units)] in file order, from `name<TAB>u,u,...` lines (the parsing of eval_ABX_clustering
    --quantized: the name loses its directory and extension).  One unit per frame: a frame token `a-b` (several groups) is refused
    by name."""
    out = []
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            if line.endswith("\n"):
                line = line[:-1]
            if not line:
                continue
            filename, frames = line.split("\t")
            name = splitext(basename(filename))[0]
            tokens = frames.split(",") if frames else []
            for token in tokens:
                if not token.isdigit():
                    raise ValueError(f"{path} line {number} ({name}): frame token '{token}' is not one unit id; several unit groups "
                                     "per frame (`a-b`) are not scored")
            out.append((name, np.array([int(t) for t in tokens], dtype=np.int32)))
    return out


def pair_lengths(names, unit_lengths, labels, max_mismatch):
    """The bookkeeping of one corpus -> (kept [(index, compared length)], skipped [name], mismatched [dict]).  labels: {name:
    sequence} or None (every utterance is kept at its own length)."""
    kept, skipped, mismatched = [], [], []
    for i, (name, n) in enumerate(zip(names, unit_lengths)):
        if labels is None:
            kept.append((i, int(n)))
        elif name not in labels:
            skipped.append(name)
        elif abs(int(n) - len(labels[name])) > max_mismatch:
            mismatched.append({"name": name, "frames": int(n), "labels": len(labels[name])})
        else:
            kept.append((i, min(int(n), len(labels[name]))))
    return kept, skipped, mismatched


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64) if len(lengths) else np.zeros(0, np.int64)


def clustering_units(args):
    """[(name, int32 units on the device)] of every audio file, assigned by cpc_kmeans_assign, and the number of centroids."""
    from .eval_ABX_clustering import ClusteringFeatures
    maker = ClusteringFeatures(args.clustering, soft_clustering=False, encoder_layer=False, keepHidden=True, group_modes="seq")
    if maker.n_groups != 1:
        raise ValueError(f"--clustering: the centroids split a frame into {maker.n_groups} groups; several unit groups per frame are "
                         "not scored")
    seqs = findAllSeqs(args.path_audio_data, extension=args.file_extension, loadCache=False)[0]
    seqs = sorted(seqs, key=lambda x: splitext(basename(x[1]))[0])
    if args.pathSeqs is not None:
        seqs = filterSeqs(args.pathSeqs, seqs)
    out = []
    for _speaker, rel in seqs:
        out.append((splitext(basename(rel))[0], maker.unit_function(os.path.join(args.path_audio_data, rel)).to(torch.int32)))
    return out, maker.n_clusters


def main(argv):
    args = check_args(parse_args(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available: unit_quality makes its counts on the "
                           "device. There is no CPU fallback.")
    device = torch.device("cuda")
    labels = None
    seen_phones = 1
    if args.pathPhone is not None:
        labels, seen_phones = parseSeqLabels(args.pathPhone)
        labels.pop("step", None)
    if args.quantized is not None:
        items = read_quantized(args.quantized)
        if args.pathSeqs is not None:
            with open(args.pathSeqs) as f:
                wanted = {splitext(basename(line.strip()))[0] for line in f if line.strip()}
            items = [it for it in items if it[0] in wanted]
        seen_units = max((int(u.max()) for _n, u in items if len(u)), default=-1) + 1
    else:
        items, seen_units = clustering_units(args)
    if not items:
        raise ValueError("no utterance to score")
    n_units = args.n_units if args.n_units is not None else max(seen_units, 1)
    n_phones = args.n_phones if args.n_phones is not None else seen_phones
    if not 1 <= n_units <= us.MAX_UNITS or not 1 <= n_phones <= us.MAX_PHONES:
        raise ValueError(f"{n_units} units and {n_phones} phones: the kernel takes 1 .. {us.MAX_UNITS} units and 1 .. "
                         f"{us.MAX_PHONES} phones")
    names = [n for n, _u in items]
    kept, skipped, mismatched = pair_lengths(names, [len(u) for _n, u in items], labels, args.max_length_mismatch)
    if not kept:
        raise ValueError("no utterance left to score: every one was skipped (no labels) or mismatched")

    counts = None
    for start in range(0, len(kept), BATCH_UTTERANCES):
        batch = kept[start:start + BATCH_UTTERANCES]
        pieces = [items[i][1] for i, _n in batch]
        unit_len = np.array([len(p) for p in pieces], dtype=np.int64)
        if isinstance(pieces[0], torch.Tensor):
            units = torch.cat(pieces).to(device)
        else:
            units = torch.from_numpy(np.concatenate(pieces).astype(np.int32)).to(device)
        lab = lab_off = None
        if labels is not None:
            rows = [np.asarray(labels[names[i]], dtype=np.int32) for i, _n in batch]
            lab = torch.from_numpy(np.concatenate(rows)).to(device)
            lab_off = torch.from_numpy(_offsets(np.array([len(r) for r in rows], dtype=np.int64))).to(device)
        if units.numel() == 0:                           # (only utterances of no frame: nothing to count, keep a valid pointer)
            units = torch.zeros(1, dtype=torch.int32, device=device)
        if lab is not None and lab.numel() == 0:
            lab = torch.zeros(1, dtype=torch.int32, device=device)
        lengths = torch.tensor([n for _i, n in batch], dtype=torch.int32, device=device)
        counts = us.count(units, lab, torch.from_numpy(_offsets(unit_len)).to(device), lab_off, lengths, n_units, n_phones,
                          tol=args.tolerance, into=counts)

    result = us.scores(counts, args.feature_size)
    joint = counts.joint.cpu().numpy()
    mapping = us.unit_to_phone(counts)
    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    report = {"args": vars(args), "scores": result, "n_utterances": len(kept), "n_frames": int(joint.sum()), "n_units": n_units,
              "n_phones": n_phones, "unit_frames": [int(v) for v in joint.sum(axis=1)],
              "phone_frames": [int(v) for v in joint.sum(axis=0)], "skipped": skipped, "mismatched": mismatched}
    with open(out_dir / "unit_scores.json", "w") as f:
        json.dump(report, f, indent=2)
    np.save(out_dir / "joint_counts.npy", joint)
    with open(out_dir / "unit_to_phone.txt", "w") as f:
        for z, y, c, tot, purity in mapping:
            f.write(f"{z} {y} {c} {tot} {purity!r}\n")
    line = (f"{len(kept)} utterances, {result['n_frames']} frames, {result['used_units']} of {n_units} units used: H {result['H_unit']:.4f} "
            f"bits, {result['bitrate_frames']:.2f} bits/s by frames, {result['bitrate_runs']:.2f} by runs")
    if labels is not None:
        line += (f"; phone purity {result['phone_purity']:.4f}, cluster purity {result['cluster_purity']:.4f}, PNMI {result['pnmi']:.4f}, "
                 f"boundary R-value {result['boundaries']['strict']['rval']:.4f}")
    print(line)
    return {"scores": result, "names": [names[i] for i, _n in kept], "skipped": skipped, "mismatched": mismatched}


if __name__ == "__main__":
    main(sys.argv[1:])
