"""Quantize every audio file of a dataset into duration-penalized unit segments (cpc2_amd/unit_segmentation.py, csrc/unit_dp.hip;
DESIGN.md section 27): for each penalty the unit sequence that minimises the summed distance to the centroids plus the penalty per
segment (Kamper & van Niekerk, Interspeech 2021, linear penalty).  The reference has no such tool; the command line is
clustering_quantization's plus --penalty.

    python -m cpc2_amd.clustering.segment_quantization <clustering dir>/checkpoint_last.pt AUDIO_DIR OUT_DIR --penalty L [L ...]
           [--file_extension .flac] [--max_size_seq 10240] [--strict True] [--nobatch] [--recursionLevel 1] [--debug] [--split i-n]

Features and distances (cpc_kmeans_distances) are computed once per file and all penalties go through one launch.  Written:
    OUT_DIR/penalty_<repr(L)>/quantized_outputs.txt   one unit per FRAME, exactly the file clustering_quantization writes (--penalty 0
                                                      reproduces it byte for byte); eval_ABX_clustering --quantized and
                                                      unit_quality --quantized read it unchanged
    OUT_DIR/penalty_<repr(L)>/unit_runs.txt           one line per file: name<TAB>unit:length,unit:length,...
    OUT_DIR/segmentation_log.json                     per penalty: frames, segments, mean run length, summed distortion and energy,
                                                      the stream's entropy and bitrate by runs (cpc2_amd.unit_scores), the files with
                                                      a non-zero status by name; once: the mean frame-wise minimum distance, the scale
                                                      lambda is read against
A file with a non-zero status (no frame, or a non-finite distance) is left out of the two text files and named in the log.

Refused before any audio is read, naming the argument: a non-empty OUT_DIR, a negative, non-finite or repeated --penalty, more than 16
of them, --file_extension .mp3, --separate-speaker, a clustering run made with --dimReduction, a codebook of several groups
(nGroups > 1).
"""
import argparse
import json
import math
import os
import sys
from pathlib import Path
from time import perf_counter

import numpy as np
import torch

from .. import unit_scores as us
from .. import unit_segmentation as seg
from ..dataset import findAllSeqs
from .clustering_quantization import format_output, quant_line, readArgs, split_bounds

BATCH_UTTERANCES = 1 << 16        # utterances per call of unit_scores.count


def parseArgs(argv):
    parser = argparse.ArgumentParser(description="Quantize audio files into duration-penalized unit segments.")
    parser.add_argument("pathCheckpoint", type=str, help="Path to the clustering checkpoint.")
    parser.add_argument("pathDB", type=str, help="Path to the dataset that we want to quantize.")
    parser.add_argument("pathOutput", type=str, help="Path to the output directory (empty or absent).")
    parser.add_argument("--penalty", type=float, nargs="+", required=True,
                        help="Charge per segment, in the unit of the squared distances; up to 16 values, all through one launch.")
    parser.add_argument("--split", type=str, default=None,
                        help="Quantize one split of the dataset: idxSplit-numSplits (idxSplit > 0), eg. --split 1-20.")
    parser.add_argument("--file_extension", type=str, default=".flac", help="Audio file extension (default: .flac).")
    parser.add_argument("--max_size_seq", type=int, default=10240,
                        help="Samples per model call when computing features (default: 10240).")
    parser.add_argument("--strict", type=bool, default=True,
                        help="Each model call sees exactly max_size_seq samples (default: True; any given value is True).")
    parser.add_argument("--debug", action="store_true", help="Quantize at most 20 files.")
    parser.add_argument("--nobatch", action="store_true",
                        help="Keep the recurrent state from chunk to chunk (model.gAR.keepHidden = True).")
    parser.add_argument("--recursionLevel", type=int, default=1, help="Speaker level in pathDB (default: 1).")
    parser.add_argument("--separate-speaker", action="store_true", help="Not supported here.")
    parser.add_argument("--time_stages", action="store_true",
                        help="Synchronise the device after every stage and write the seconds per stage into the log.")
    return parser.parse_args(argv)


def check_args(args):
    """The refusals that need nothing but the command line, each naming its argument."""
    if os.path.exists(args.pathOutput) and (not os.path.isdir(args.pathOutput) or os.listdir(args.pathOutput)):
        raise ValueError(f"OUT_DIR {args.pathOutput} exists and is not an empty directory: the tool writes its files there and "
                         "overwrites nothing")
    if len(args.penalty) > seg.MAX_PENALTIES:
        raise ValueError(f"--penalty: {len(args.penalty)} values; at most {seg.MAX_PENALTIES} go through one launch")
    for v in args.penalty:
        if not (math.isfinite(v) and v >= 0):
            raise ValueError(f"--penalty {v!r} must be finite and >= 0")
    if len({repr(float(v)) for v in args.penalty}) != len(args.penalty):
        raise ValueError(f"--penalty {args.penalty}: a value is repeated; every penalty writes a directory of its own")
    if args.file_extension.lower() == ".mp3":
        raise NotImplementedError("--file_extension .mp3: there is no mp3 decoder in this package; convert the files to .wav or .flac")
    if args.separate_speaker:
        raise NotImplementedError("--separate-speaker is not supported (clustering_quantization refuses it too)")
    if args.split:
        parts = args.split.split("-")
        if not (len(parts) == 2 and all(p.isdigit() for p in parts) and int(parts[1]) >= int(parts[0]) >= 1):
            raise ValueError("--split must be under the form idxSplit-numSplits (numSplits >= idxSplit >= 1), eg. --split 1-20")
    if not args.pathCheckpoint.endswith(".pt"):
        raise ValueError(f"CLUSTER_CKPT {args.pathCheckpoint} must be a .pt checkpoint of clustering_script")
    return args


def check_clustering_args(clustering_args):
    """The refusals that need the clustering run's args.json."""
    if getattr(clustering_args, "dimReduction", None) is not None:
        raise NotImplementedError("CLUSTER_CKPT: the clustering run used --dimReduction, which is not supported")
    if int(getattr(clustering_args, "nGroups", 1) or 1) > 1:
        raise NotImplementedError(f"CLUSTER_CKPT: the codebook splits a frame into nGroups = {clustering_args.nGroups} groups; several "
                                  "groups per frame are not segmented")


def runs_line(unit, length):
    return ",".join(f"{int(z)}:{int(n)}" for z, n in zip(unit, length))


def main(argv):
    args = check_args(parseArgs(argv))
    pens = [float(v) for v in args.penalty]
    clustering_args = readArgs(Path(args.pathCheckpoint).parent)
    check_clustering_args(clustering_args)
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available: segment_quantization makes its units "
                           "on the device. There is no CPU fallback.")
    from ..feature_loader import FeatureModule, buildFeature, loadModel
    from .clustering import kmeans_distances, loadClusterModule

    print(f"Looking for all {args.file_extension} files in {args.pathDB} with speakerLevel {args.recursionLevel}")
    seqNames, speakers = findAllSeqs(args.pathDB, speaker_level=args.recursionLevel, extension=args.file_extension)
    print(f"Done! Found {len(seqNames)} files and {len(speakers)} speakers!")
    suffix = ""
    if args.split:
        idx_split, num_splits = (int(p) for p in args.split.split("-"))
        startIdx, endIdx = split_bounds(len(seqNames), idx_split, num_splits)
        seqNames = seqNames[startIdx:endIdx]
        suffix = f"_split_{idx_split}-{num_splits}"
        print(f"Quantizing split {idx_split} out of {num_splits} splits, with {len(seqNames)} files "
              f"(idx in range({startIdx}, {endIdx})).")
    if args.debug:
        seqNames = seqNames[:20]

    clusterModule = loadClusterModule(args.pathCheckpoint)
    Ck = clusterModule.Ck
    if Ck.dim() == 3 and Ck.size(0) != 1:
        raise NotImplementedError(f"CLUSTER_CKPT: centroids of shape {tuple(Ck.shape)}; one codebook [1, K, D] is segmented")
    k, d = Ck.size(-2), Ck.size(-1)
    level_gru = getattr(clustering_args, "level_gru", None)
    updateConfig = argparse.Namespace(nLevelsGRU=level_gru) if level_gru is not None else None
    model = loadModel([clustering_args.pathCheckpoint], updateConfig=updateConfig)[0]
    if args.nobatch:
        model.gAR.keepHidden = True
    featureMaker = FeatureModule(model, clustering_args.encoder_layer)
    if not clustering_args.train_mode:
        featureMaker.eval()
    featureMaker.cuda()
    device = torch.device("cuda", torch.cuda.current_device())

    n_pen = len(pens)
    lines = [[] for _ in pens]
    run_lines = [[] for _ in pens]
    kept_names, kept_units = [], [[] for _ in pens]
    flagged = [[] for _ in pens]
    frames = 0
    segments = torch.zeros(n_pen, dtype=torch.int64, device=device)
    energy = torch.zeros(n_pen, dtype=torch.float64, device=device)
    distortion = [0.0] * n_pen
    min_sum = torch.zeros(1, dtype=torch.float64, device=device)
    seconds = {"features": 0.0, "distances": 0.0, "segmentation": 0.0, "lines": 0.0}

    def lap(stage, t0):
        if args.time_stages:
            torch.cuda.synchronize()
        seconds[stage] += perf_counter() - t0
        return perf_counter()

    one_off = torch.zeros(1, dtype=torch.int64, device=device)
    for vals in seqNames:
        t0 = perf_counter()
        cFeatures = buildFeature(featureMaker, os.path.join(args.pathDB, vals[1]), seqNorm=False, strict=args.strict).cuda()
        if cFeatures.size(-1) != d:
            raise NotImplementedError(f"CLUSTER_CKPT: features of width {cFeatures.size(-1)} against centroids of width {d}: a codebook "
                                      "of several groups (nGroups > 1) is not segmented")
        t0 = lap("features", t0)
        cost = kmeans_distances(cFeatures.view(-1, d), Ck)
        n = cost.size(0)
        t0 = lap("distances", t0)
        units, e, s, status = seg.segment_costs(cost, one_off, torch.tensor([n], dtype=torch.int32, device=device), pens)
        t0 = lap("segmentation", t0)
        status = status[:, 0].cpu().tolist()
        name = os.path.splitext(os.path.basename(vals[1]))[0]
        if any(status):
            for p in range(n_pen):
                flagged[p].append({"name": name, "status": int(status[p])})
            continue
        frames += n
        min_sum += cost.min(dim=1).values.double().sum()
        segments += s[:, 0]
        energy += e[:, 0]
        host = units.cpu().numpy()
        kept_names.append(vals)
        for p in range(n_pen):
            distortion[p] += seg.distortion(cost, units[p])
            lines[p].append(quant_line(host[p].tolist(), 1))
            unit, _start, length = seg.runs(host[p], [0], [n])[0]
            run_lines[p].append(runs_line(unit, length))
            kept_units[p].append(units[p])
        lap("lines", t0)

    out_dir = Path(args.pathOutput)
    out_dir.mkdir(parents=True, exist_ok=True)
    segments, energy = segments.cpu().tolist(), energy.cpu().tolist()
    log = {"args": vars(args), "n_files": len(kept_names), "n_frames": frames, "n_units": int(k),
           "mean_min_distance": float(min_sum.item()) / frames if frames else None, "penalties": []}
    lengths = np.array([u.numel() for u in kept_units[0]], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64) if len(lengths) else np.zeros(0, np.int64)
    for p, lam in enumerate(pens):
        pdir = out_dir / f"penalty_{lam!r}"
        pdir.mkdir()
        with open(pdir / f"quantized_outputs{suffix}.txt", "w") as f:
            f.write(format_output(kept_names, lines[p]))
        with open(pdir / f"unit_runs{suffix}.txt", "w") as f:
            f.write(format_output(kept_names, run_lines[p]))
        rec = {"penalty": lam, "frames": frames, "segments": int(segments[p]),
               "mean_run_length": frames / segments[p] if segments[p] else None, "distortion": distortion[p], "energy": energy[p],
               "flagged": flagged[p]}
        if frames:
            counts = None
            for start in range(0, len(lengths), BATCH_UTTERANCES):
                stop = min(start + BATCH_UTTERANCES, len(lengths))
                pack = torch.cat(kept_units[p][start:stop])
                counts = us.count(pack, None, torch.from_numpy(offsets[start:stop] - offsets[start]), None,
                                  torch.from_numpy(lengths[start:stop].astype(np.int32)), int(k), 1, into=counts)
            sc = us.scores(counts)
            rec.update({"H_unit": sc["H_unit"], "used_units": sc["used_units"], "bitrate_frames": sc["bitrate_frames"],
                        "bitrate_runs": sc["bitrate_runs"], "n_unit_runs": sc["n_unit_runs"]})
        log["penalties"].append(rec)
        print(f"penalty {lam!r}: {frames} frames in {rec['segments']} segments"
              + (f", {rec['bitrate_runs']:.2f} bits/s by runs" if frames else ""))
    if args.time_stages:
        log["seconds"] = seconds
    with open(out_dir / "segmentation_log.json", "w") as f:
        json.dump(log, f, indent=2)
    return log


if __name__ == "__main__":
    main(sys.argv[1:])
