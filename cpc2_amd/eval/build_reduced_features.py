"""Write the features of every audio file of a directory behind a fitted PCA / SFA projection (cpc2_amd.dim_reduction), one output
file per input:

    python -m cpc2_amd.eval.build_reduced_features AUDIO_DIR OUT_DIR CKPT.pt DIMRED.pt [--centroidLimits A B]
           [--format pt|npy|npz|fea] [--file_extension .flac] [--maxSizeSeq 64000] [--strict] [--seqNorm]

DIMRED.pt is the file `python -m cpc2_amd.dim_reduction` (or the reference's tool) writes.  The features come through
dim_reduction.ModelDimReduced and feature_loader.buildFeature_device, and each file is written by
build_baseline_features.write_feature: --format pt is a float32 CPU tensor [T, D], what `eval_ABX from_pre_computed FILE.item
OUT_DIR --out DIR` loads; npy / npz / fea as build_zeroSpeech_features writes them.  OUT_DIR/reduced_args.json holds the arguments.

Refused by name before any audio is read: a non-empty OUT_DIR, --file_extension .mp3, a missing checkpoint or projection file, and
what loadDimReduction refuses (--centroidLimits on a PCA, or on a file without centroid_values).
"""
import argparse
import json
import os
import sys
import time

import torch

from .. import audio
from .. import dataset
from ..dim_reduction import ModelDimReduced, loadDimReduction
from ..feature_loader import FeatureModule, buildFeature_device, loadModel
from .build_baseline_features import FORMATS, write_feature

STAGES = ("decode", "model", "copy", "write")


def parse_args(argv):
    parser = argparse.ArgumentParser("Build features behind a PCA / SFA projection")
    parser.add_argument("path_audio", help="Directory of the audio files")
    parser.add_argument("path_out", help="Output directory (created; must be empty)")
    parser.add_argument("pathCheckpoint", help="Checkpoint of the CPC model")
    parser.add_argument("pathDimReduction", help="File written by python -m cpc2_amd.dim_reduction")
    parser.add_argument("--centroidLimits", type=float, nargs=2, default=None, metavar=("A", "B"),
                        help="SFA: keep the dimensions whose centroid_values lie strictly between A and B")
    parser.add_argument("--format", default="pt", choices=list(FORMATS))
    parser.add_argument("--file_extension", type=str, default=".flac")
    parser.add_argument("--maxSizeSeq", type=int, default=64000)
    parser.add_argument("--strict", action="store_true")
    parser.add_argument("--seqNorm", action="store_true")
    return parser.parse_args(argv)


def check_args(args):
    """The refusals, each naming its argument; no audio is read.  Returns the loaded projection (on the host)."""
    if args.file_extension.lower() == ".mp3":
        raise NotImplementedError("--file_extension .mp3: there is no mp3 decoder in this package; convert the files to .wav or .flac")
    if os.path.exists(args.path_out) and (not os.path.isdir(args.path_out) or os.listdir(args.path_out)):
        raise ValueError(f"{args.path_out} exists and is not an empty directory: the tool writes one file per audio file under its "
                         "stem and overwrites nothing")
    for name in ("pathCheckpoint", "pathDimReduction"):
        path = getattr(args, name)
        if not (path.endswith(".pt") and os.path.isfile(path)):
            raise ValueError(f"{name} {path}: not an existing .pt file")
    if args.maxSizeSeq < 1:
        raise ValueError(f"--maxSizeSeq {args.maxSizeSeq}: at least 1")
    return loadDimReduction(args.pathDimReduction, args.centroidLimits)


def build_all(featureMaker, path_audio, path_out, seq_list, step, fmt="pt", strict=False, maxSizeSeq=64000, seqNorm=False,
              timings=None):
    """One output file per sequence of seq_list (paths relative to path_audio), named by its stem."""
    timings = {} if timings is None else timings
    for stage in STAGES:
        timings.setdefault(stage, 0.0)
    device = next(featureMaker.parameters()).device
    seen = set()
    for seq in seq_list:
        stem = os.path.basename(os.path.splitext(seq)[0])
        if stem in seen:
            raise ValueError(f"two audio files share the stem {stem}: their feature files would overwrite each other")
        seen.add(stem)
        t0 = time.perf_counter()
        wave = audio.load(os.path.join(path_audio, seq))[0]
        t1 = time.perf_counter()
        timings["decode"] += t1 - t0
        feature = buildFeature_device(featureMaker, wave, strict=strict or seqNorm, maxSizeSeq=maxSizeSeq, seqNorm=seqNorm)
        torch.cuda.synchronize(device)
        timings["model"] += time.perf_counter() - t1
        write_feature(os.path.join(path_out, stem + "." + fmt), feature[0], fmt, step, timings)
    return timings


def main(argv):
    args = parse_args(argv)
    dimRed = check_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available: build_reduced_features runs the model "
                           "and the projection on the device. There is no CPU fallback.")
    seq_list = [x[1] for x in dataset.findAllSeqs(args.path_audio, extension=args.file_extension, loadCache=False)[0]]
    if not seq_list:
        raise ValueError(f"no {args.file_extension} file under {args.path_audio}")
    os.makedirs(args.path_out, exist_ok=True)
    with open(os.path.join(args.path_out, "reduced_args.json"), "w") as file:
        json.dump(vars(args), file, indent=2)

    model = loadModel([args.pathCheckpoint])[0]
    step = model.gEncoder.DOWNSAMPLING / 16000
    featureMaker = ModelDimReduced(FeatureModule(model, False), dimRed).cuda()
    featureMaker.eval()
    t0 = time.perf_counter()
    timings = build_all(featureMaker, args.path_audio, args.path_out, seq_list, step, fmt=args.format, strict=args.strict,
                        maxSizeSeq=args.maxSizeSeq, seqNorm=args.seqNorm)
    total = time.perf_counter() - t0
    print(f"{len(seq_list)} files in {total:.3f} s: " + ", ".join(f"{stage} {timings[stage]:.3f} s" for stage in STAGES))
    return timings


if __name__ == "__main__":
    main(sys.argv[1:])
