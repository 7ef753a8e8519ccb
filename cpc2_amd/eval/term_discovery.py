"""Unsupervised spoken term discovery of a trained CPC model or of pre-computed features (cpc2_amd/term_discovery.py,
csrc/lalign.hip).  The reference has no such tool; the command line has the shape of eval_ABX.

    python -m cpc2_amd.eval.term_discovery from_checkpoint CKPT.pt AUDIO_DIR --threshold T --out DIR [flags]
    python -m cpc2_amd.eval.term_discovery from_pre_computed FEATURE_DIR --file_extension .npy|.pt --threshold T --out DIR [flags]
    python -m cpc2_amd.eval.term_discovery from_units QUANTIZED.txt --threshold T --out DIR [--seq_list L]
           [--distance_mode cosine|euclidian] [--gap_penalty G] [--min_frames 25] [--min_score 0] [--max_frames N]
           [--pathPhone LABELS.txt] [--top K]

    flags: [--file_extension .flac] [--seq_list L] [--distance_mode cosine|euclidian] [--gap_penalty G] [--min_frames 25]
           [--min_score 0] [--max_frames N] [--seqNorm] [--pathPhone LABELS.txt] [--top K] [--seed 0]

Every file under AUDIO_DIR / FEATURE_DIR with the extension is an utterance (--seq_list: only the base names it lists).  Every
unordered pair of utterances is aligned LOCALLY by cpc_local_align (one best match per pair, both ends free on both sides); a
match is kept when both of its sides span at least --min_frames frames and its score is at least --min_score, and the matches
are ordered by descending score (--top K: the first K only).  Cosine mode normalises the rows with normalize_with_singularity, as
ABX does.

--threshold is required: there is no tuned default to offer.  It is the frame distance below which a frame pair earns gain, given
as a number, or as `qP`: the P-th percentile (0 < P < 100) of the frame distances of a seeded sample (--seed) of cross-utterance
frame pairs.  The sample's percentiles 1, 5, 10, 25 and 50 and the theta actually used are always written to the log, so that a
threshold can be chosen from a first run.  --gap_penalty (the cost of a horizontal or vertical step) defaults to theta / 2: a
stated choice, not a tuned one.

Utterances with non-finite features, without a frame or longer than --max_frames (default MAX_FRAMES_DEFAULT; the kernel's limit
is 32767) are left out and listed by name.  Written into --out:
    matches.txt             `file_a start_a end_a file_b start_b end_b score length` per match, times in seconds
    classes.txt             one two-member class per match in the ZeroSpeech layout: `Class k`, one `file start end` line per
                            member, a blank line
    discovery_scores.json   only with --pathPhone (frame labels, `name l0 l1 ...` per line): NED, coverage and the counts of
                            term_discovery.scores; their agreement with the ZeroSpeech TDE toolkit is UNMEASURED
    discovery_log.json      the arguments, the theta and gamma used, the distance percentiles, the utterances left out by name, the
                            pair and cell counts and the wall time by stage

from_units searches QUANTIZED units (csrc/lalign_units.hip): QUANTIZED.txt is the quantized_outputs.txt
that clustering_quantization and segment_quantization write (or the directory that holds one), read by
unit_quality.read_quantized: an utterance is a line of it.  The frame distance is then one of two numbers, those the chosen
--distance_mode gives on one-hot rows (d_same = 0 and d_diff = 0.5 for cosine, 0 and sqrt 2 for euclidian), and
cpc_local_align_units runs the same recurrence on the unit ids.  Matches, scores and files are made by the same code; the log also
names the source, the number of distinct units and the two distances, and has no distance percentiles: there is no sample.
Refused with from_units, by flag: --seqNorm; --threshold qP (a percentile of a distance that takes two values says nothing); a
--threshold outside (d_same, d_diff]: at or below d_same no cell can gain, above d_diff every cell gains and the match is the whole
matrix.

Refused by name before any audio or feature file is opened: a non-empty --out, --file_extension .mp3, a malformed --threshold, a
negative --gap_penalty, --min_frames or --min_score, a --max_frames above the kernel's limit, --top < 1.
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

from .. import term_discovery as tdisc
from ..dataset import parseSeqLabels
from .ABX.abx_iterators import normalize_with_singularity
from .term_detection import _listing, feature_loader, format_time, read_units, unit_distances, units_file

STAGES = ("decode", "model", "copy", "threshold", "kernels", "select", "score", "write")
MAX_FRAMES_DEFAULT = 16384         # utterances the scratch is sized for by default: 24 bytes x frames per workgroup
PERCENTILES = (1, 5, 10, 25, 50)
SAMPLE_PAIRS = 200_000             # cross-utterance frame pairs drawn for the distance percentiles


def _common(parser):
    parser.add_argument('--threshold', type=str, required=True, help="theta: a number, or qP = the P-th percentile of sampled frame distances")
    parser.add_argument('--out', type=str, required=True, help="Directory the results are written into (empty or absent)")
    parser.add_argument('--seq_list', type=str, default=None, help="List of the utterances to search (base names)")
    parser.add_argument('--distance_mode', type=str, default='cosine', choices=['cosine', 'euclidian'])
    parser.add_argument('--gap_penalty', type=float, default=None, help="gamma, the cost of a horizontal or vertical step (default theta / 2)")
    parser.add_argument('--min_frames', type=int, default=25, help="Shortest side of a kept match, in frames")
    parser.add_argument('--min_score', type=float, default=0.0, help="Smallest score of a kept match")
    parser.add_argument('--max_frames', type=int, default=MAX_FRAMES_DEFAULT, help="Longer utterances are left out and listed")
    parser.add_argument('--seqNorm', action='store_true', help="Normalize each file's features across the time channel")
    parser.add_argument('--pathPhone', type=str, default=None, help="Frame-level phone labels, `name l0 l1 ...` per line")
    parser.add_argument('--top', type=int, default=None, help="Keep the K best matches only")
    parser.add_argument('--seed', type=int, default=0, help="Seed of the frame-pair sample behind the distance percentiles")


def parse_args(argv):
    base_parser = argparse.ArgumentParser(description='Unsupervised spoken term discovery')
    subparsers = base_parser.add_subparsers(dest='load')
    ckpt = subparsers.add_parser('from_checkpoint')
    ckpt.add_argument('path_checkpoint', type=str, help="Path to the model's checkpoint")
    ckpt.add_argument('path_dataset', type=str, help="Path to the audio files")
    ckpt.add_argument('--file_extension', type=str, default='.flac', help=".wav or .flac (.mp3 is refused)")
    ckpt.add_argument('--get_encoded', action='store_true', help="Use the output of the encoder network")
    ckpt.add_argument('--max_size_seq', default=64000, type=int, help="Samples per model call")
    ckpt.add_argument('--strict', action='store_true', help="Each model call takes exactly max_size_seq samples")
    _common(ckpt)
    pre = subparsers.add_parser('from_pre_computed')
    pre.add_argument('path_dataset', type=str, help="Path to pre-computed [frames, dim] features")
    pre.add_argument('--file_extension', type=str, default='.pt', help=".pt or .npy")
    _common(pre)
    units = subparsers.add_parser('from_units')
    units.add_argument('path_units', type=str, help="quantized_outputs.txt of clustering_quantization / segment_quantization")
    _common(units)
    args = base_parser.parse_args(argv)
    if args.load is None:
        base_parser.error("choose from_checkpoint, from_pre_computed or from_units")
    return args


def parse_threshold(text):
    """--threshold as ("value", theta) or ("percentile", P); anything else is refused by name."""
    try:
        if text[:1] in ("q", "Q"):
            p = float(text[1:])
            if not (math.isfinite(p) and 0 < p < 100):
                raise ValueError
            return "percentile", p
        theta = float(text)
        if not (math.isfinite(theta) and theta > 0):
            raise ValueError
        return "value", theta
    except ValueError:
        raise ValueError(f"--threshold {text}: give a finite number > 0, or qP with 0 < P < 100 (the P-th percentile of sampled "
                         "frame distances)") from None


def check_args(args):
    """The refusals, each naming its flag; no audio or feature file has been opened.  Leaves the parsed threshold in
    args.threshold_kind / args.threshold_value."""
    if args.load == 'from_units':
        if args.seqNorm:
            raise ValueError("--seqNorm with from_units: units are not features, there is nothing to normalise")
    else:
        ext = args.file_extension.lower()
        if ext == ".mp3":
            raise NotImplementedError("--file_extension .mp3: there is no mp3 decoder in this package; convert the files to .wav or .flac")
        allowed = (".wav", ".flac") if args.load == 'from_checkpoint' else (".pt", ".npy")
        if ext not in allowed:
            raise ValueError(f"--file_extension {args.file_extension}: {args.load} reads {' or '.join(allowed)}")
    args.threshold_kind, args.threshold_value = parse_threshold(args.threshold)
    if args.load == 'from_units':
        if args.threshold_kind == "percentile":
            raise ValueError(f"--threshold {args.threshold} with from_units: the frame distance of two units takes two values, a "
                             "percentile of it says nothing; give a number")
        d_same, d_diff = unit_distances(args.distance_mode)
        if not d_same < float(np.float32(args.threshold_value)) <= d_diff:
            raise ValueError(f"--threshold {args.threshold} with from_units: must lie in (d_same, d_diff] = ({d_same:.6g}, {d_diff:.6g}] of "
                             f"--distance_mode {args.distance_mode}: at or below d_same no cell can gain, above d_diff every cell gains "
                             "and the match is the whole matrix")
    if args.gap_penalty is not None and not (math.isfinite(args.gap_penalty) and args.gap_penalty >= 0):
        raise ValueError(f"--gap_penalty {args.gap_penalty} must be finite and >= 0")
    if args.min_frames < 0:
        raise ValueError(f"--min_frames {args.min_frames} must be >= 0")
    if not args.min_score >= 0 or not math.isfinite(args.min_score):
        raise ValueError(f"--min_score {args.min_score} must be finite and >= 0")
    if not 1 <= args.max_frames <= tdisc.MAX_FRAMES:
        raise ValueError(f"--max_frames {args.max_frames}: the kernel takes utterances of 1 .. {tdisc.MAX_FRAMES} frames")
    if args.top is not None and args.top < 1:
        raise ValueError(f"--top {args.top} must be >= 1")
    if os.path.exists(args.out) and (not os.path.isdir(args.out) or os.listdir(args.out)):
        raise ValueError(f"--out {args.out} exists and is not an empty directory: the tool writes its files there and overwrites "
                         "nothing")
    if args.load == 'from_units':
        args.path_units = units_file(args.path_units)
    return args


def sample_distances(frames, offs, lens, distance_mode, seed, n_pairs=SAMPLE_PAIRS):
    """The frame distances of n_pairs seeded draws of a frame pair from two DIFFERENT utterances (float64 numpy, sorted).  A
    sample for choosing a threshold, made with torch on the device; the alignment itself never uses it."""
    rng = np.random.default_rng(seed)
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(offs)
    a = rng.integers(0, n, n_pairs)
    b = (a + rng.integers(1, n, n_pairs)) % n                     # another utterance
    ia = offs[a] + (rng.random(n_pairs) * lens[a]).astype(np.int64)
    ib = offs[b] + (rng.random(n_pairs) * lens[b]).astype(np.int64)
    x = frames[torch.from_numpy(ia).to(frames.device)].double()
    y = frames[torch.from_numpy(ib).to(frames.device)].double()
    if distance_mode == "cosine":
        d = torch.acos(torch.clamp((x * y).sum(1), -1.0, 1.0)) / math.pi
    else:
        d = (x - y).norm(dim=1)
    return np.sort(d.cpu().numpy())


def main(argv):
    args = check_args(parse_args(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available: term_discovery makes the frame "
                           "distances and the local alignment on the device. There is no CPU fallback.")
    timings = {stage: 0.0 for stage in STAGES}
    from_units = args.load == 'from_units'
    if from_units:
        # a "path" is the utterance's name and its "features" are the line's unit ids (int32 numpy)
        t0 = time.perf_counter()
        paths = dict(read_units(args.path_units, "from_units"))
        if args.seq_list is not None:
            with open(args.seq_list, 'r') as f:
                wanted = {p.strip() for p in f.readlines() if p.strip()}
            paths = {name: units for name, units in paths.items() if name in wanted}
        paths = {name: paths[name] for name in sorted(paths)}
        timings["decode"] += time.perf_counter() - t0
        if not paths:
            raise ValueError(f"from_units {args.path_units}: no utterance" + (" named in --seq_list" if args.seq_list else ""))

        def load(units):
            return units
    else:
        paths = _listing(args.path_dataset, args.file_extension, args.seq_list)
        if not paths:
            raise ValueError(f"no {args.file_extension} file found under {args.path_dataset}")
        load = feature_loader(args, timings)
    cosine = args.distance_mode == 'cosine'

    # ---- features: every file once; items are spans of one frames buffer ----
    pieces, names, offs, lens, n_rows, dim = [], [], [], [], 0, None
    non_finite, too_long, empty = [], [], []
    for name, path in paths.items():
        feats = load(path)
        if not from_units:
            if dim is None:
                dim = feats.size(1)
            if feats.size(1) != dim:
                raise ValueError(f"{path}: {feats.size(1)} feature columns, the files before it have {dim}")
        if len(feats) < 1:
            empty.append(name)
        elif len(feats) > args.max_frames:
            too_long.append(name)
        elif not from_units and not bool(torch.isfinite(feats).all()):
            non_finite.append(name)
        else:
            if cosine and not from_units:
                feats = normalize_with_singularity(feats)
            names.append(name)
            offs.append(n_rows)
            lens.append(len(feats))
            pieces.append(feats)
            n_rows += len(feats)
    if len(names) < 2:
        raise ValueError("fewer than two utterances left to compare: the others were empty, non-finite or longer than --max_frames")

    t0 = time.perf_counter()
    device = torch.device("cuda")
    if from_units:
        all_units = np.concatenate(pieces).astype(np.int32)
        source_log = dict(zip(("d_same", "d_diff"), unit_distances(args.distance_mode)))
        source_log.update(source="from_units", distinct_units=int(np.unique(all_units).size))
        frames = torch.from_numpy(all_units).to(device)
        dp = 0
    else:
        source_log = {"source": args.load}
        width = pieces[0].size(1)
        dp = -(-width // 4) * 4
        frames = torch.zeros(n_rows, dp, dtype=torch.float32, device=device)
        frames[:, :width] = torch.cat(pieces, 0)
    del pieces
    item_off = torch.tensor(offs, dtype=torch.int32, device=device)
    item_len = torch.tensor(lens, dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    timings["copy"] += time.perf_counter() - t0

    # ---- theta and gamma ----
    t0 = time.perf_counter()
    sample = np.zeros(0) if from_units else sample_distances(frames, offs, lens, args.distance_mode, args.seed)
    percentiles = {} if from_units else {str(p): float(np.percentile(sample, p)) for p in PERCENTILES}
    theta = args.threshold_value if args.threshold_kind == "value" else float(np.percentile(sample, args.threshold_value))
    theta = float(np.float32(theta))
    if not (math.isfinite(theta) and theta > 0):
        raise ValueError(f"--threshold {args.threshold}: the percentile is {theta}, not a positive distance")
    gamma = float(np.float32(theta / 2 if args.gap_penalty is None else args.gap_penalty))
    timings["threshold"] += time.perf_counter() - t0
    if not from_units:
        print("frame distance percentiles of the sample: " + ", ".join(f"{p} %: {v:.4f}" for p, v in percentiles.items()))
    print(f"theta {theta:.6g} gamma {gamma:.6g}")

    # ---- every pair ----
    t0 = time.perf_counter()
    if from_units:
        score, span, pair_a, pair_b = tdisc.local_alignment_units(frames, item_off, item_len, np.arange(len(names)),
                                                                  source_log["d_same"], source_log["d_diff"], theta, gamma,
                                                                  lens_host=lens)
    else:
        score, span, pair_a, pair_b = tdisc.local_alignment(frames, item_off, item_len, np.arange(len(names)), args.distance_mode,
                                                            theta, gamma, lens_host=lens)
    torch.cuda.synchronize()
    timings["kernels"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    score_h, span_h = score.cpu().numpy(), span.cpu().numpy()
    timings["copy"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    kept = tdisc.select(score_h, span_h, args.min_frames, args.min_score)
    n_selected = len(kept)
    if args.top is not None:
        kept = kept[:args.top]
    matches = [(names[pair_a[p]], int(span_h[p, 0]), int(span_h[p, 1]), names[pair_b[p]], int(span_h[p, 2]), int(span_h[p, 3]))
               for p in kept]
    timings["select"] += time.perf_counter() - t0

    result = None
    if args.pathPhone is not None:
        t0 = time.perf_counter()
        labels = parseSeqLabels(args.pathPhone)[0]
        labels.pop("step", None)
        result = tdisc.scores(matches, labels, dict(zip(names, lens)))
        result["args"] = {k: v for k, v in vars(args).items()}
        result["theta"], result["gamma"] = theta, gamma
        torch.cuda.synchronize()
        timings["score"] += time.perf_counter() - t0

    t0 = time.perf_counter()
    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "matches.txt", "w") as f:
        for p, (fa, sa, ea, fb, sb, eb) in zip(kept, matches):
            f.write(f"{fa} {format_time(sa)} {format_time(ea + 1)} {fb} {format_time(sb)} {format_time(eb + 1)} "
                    f"{float(score_h[p]):.8g} {int(span_h[p, 4])}\n")
    with open(out_dir / "classes.txt", "w") as f:
        for k, (fa, sa, ea, fb, sb, eb) in enumerate(matches):
            f.write(f"Class {k}\n{fa} {format_time(sa)} {format_time(ea + 1)}\n{fb} {format_time(sb)} {format_time(eb + 1)}\n\n")
    if result is not None:
        with open(out_dir / "discovery_scores.json", "w") as f:
            json.dump(result, f, indent=2)
    timings["write"] += time.perf_counter() - t0
    lens64 = np.asarray(lens, dtype=np.int64)
    log = {"args": {k: v for k, v in vars(args).items()}, "theta": theta, "gamma": gamma, "distance_percentiles": percentiles,
           "sampled_frame_pairs": int(len(sample)), "utterances": len(names), "pairs": int(len(pair_a)),
           "cells": int((lens64[pair_a] * lens64[pair_b]).sum()), "frames": int(n_rows), "feature_columns": int(dp), **source_log,
           "pairs_with_a_match": int((score_h > 0).sum()), "matches_selected": int(n_selected), "matches_written": len(matches),
           "empty": empty, "too_long": too_long, "non_finite": non_finite, "seconds": timings}
    with open(out_dir / "discovery_log.json", "w") as f:
        json.dump(log, f, indent=2)
    print(f"{len(names)} utterances, {len(pair_a)} pairs, {len(matches)} matches written"
          + (f"; NED {result['ned']:.4f} coverage {result['coverage']:.4f}" if result is not None else ""))
    print(", ".join(f"{stage} {timings[stage]:.3f} s" for stage in STAGES))
    return {"scores": result, "log": log, "names": names, "score": score_h, "span": span_h, "pair_a": pair_a, "pair_b": pair_b,
            "kept": kept, "matches": matches, "theta": theta, "gamma": gamma}


if __name__ == "__main__":
    main(sys.argv[1:])
