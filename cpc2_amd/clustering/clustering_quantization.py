"""Quantize every audio file of a dataset into discrete units with a clustering checkpoint -- cpc/clustering/
clustering_quantization.py of the reference: same command line (including --strict's type=bool, under which any given
value is True), same output file, one line per file:

    <file name without extension>\\t<frame>,<frame>,...      a frame = its nGroups unit ids joined with "-"

lines joined with "\\n", no trailing newline.

    python -m cpc2_amd.clustering.clustering_quantization <clustering dir>/checkpoint_last.pt <dataset dir> <output dir>

Units come from the fused assign kernel (kMeanCluster.assign) on the GPU, for files of any length: there is no CPU branch.
--separate-speaker is refused up front (the reference computes everything, then fails: its output file is never named
on that path).
"""
import argparse
import json
import os
import sys
from pathlib import Path
from time import time

from ..dataset import findAllSeqs
from ..feature_loader import FeatureModule, buildFeature, loadModel
from .clustering import loadClusterModule


def readArgs(path_dir):
    print(f"Loading args from {path_dir}")
    with open(Path(path_dir) / "args.json", "r") as file:
        return argparse.Namespace(**json.load(file))


def parseArgs(argv):
    parser = argparse.ArgumentParser(description="Quantize audio files using CPC Clustering Module.")
    parser.add_argument("pathCheckpoint", type=str, help="Path to the clustering checkpoint.")
    parser.add_argument("pathDB", type=str, help="Path to the dataset that we want to quantize.")
    parser.add_argument("pathOutput", type=str, help="Path to the output directory.")
    parser.add_argument("--split", type=str, default=None,
                        help="Quantize one split of the dataset: idxSplit-numSplits (idxSplit > 0), eg. --split 1-20.")
    parser.add_argument("--file_extension", type=str, default=".flac", help="Audio file extension (default: .flac).")
    parser.add_argument("--max_size_seq", type=int, default=10240,
                        help="Samples per model call when computing features (default: 10240).")
    parser.add_argument("--batch_size", type=int, default=8, help="Batch size of the feature computation (default: 8).")
    parser.add_argument("--strict", type=bool, default=True,
                        help="Each model call sees exactly max_size_seq samples (default: True; any given value is True).")
    parser.add_argument("--debug", action="store_true", help="Quantize at most 20 files.")
    parser.add_argument("--nobatch", action="store_true",
                        help="Keep the recurrent state from chunk to chunk (model.gAR.keepHidden = True).")
    parser.add_argument("--recursionLevel", type=int, default=1, help="Speaker level in pathDB (default: 1).")
    parser.add_argument("--separate-speaker", action="store_true", help="Not supported here.")
    return parser.parse_args(argv)


def split_bounds(n_seqs, idx_split, num_splits):
    """[start, end) of split idx_split (1-based) out of num_splits; the last split takes the remainder."""
    start = n_seqs // num_splits * (idx_split - 1)
    end = n_seqs if idx_split == num_splits else min(n_seqs // num_splits * idx_split, n_seqs)
    return start, end


def quant_line(units, nGroups):
    """The units of one file ([frames * nGroups] ints) as the reference writes them."""
    return ",".join("-".join(str(int(i)) for i in units[f:f + nGroups]) for f in range(0, len(units), nGroups))


def format_output(seqNames, seqQuantLines):
    return "\n".join("\t".join([os.path.splitext(os.path.basename(vals[1]))[0], line])
                     for vals, line in zip(seqNames, seqQuantLines))


def main(argv):
    args = parseArgs(argv)
    if args.separate_speaker:
        raise SystemExit("--separate-speaker is not supported (the reference never names its output file on that path).")

    print("=============================================================")
    print(f"Quantizing data from {args.pathDB}")
    print("=============================================================")

    if not os.path.exists(args.pathOutput):
        print("")
        print(f"Creating the output directory at {args.pathOutput}")
        Path(args.pathOutput).mkdir(parents=True, exist_ok=True)

    if args.split:
        parts = args.split.split("-")
        assert len(parts) == 2 and int(parts[1]) >= int(parts[0]) >= 1, \
            "SPLIT must be under the form idxSplit-numSplits (numSplits >= idxSplit >= 1), eg. --split 1-20"
        idx_split, num_splits = int(parts[0]), int(parts[1])

    print("")
    print(f"Looking for all {args.file_extension} files in {args.pathDB} with speakerLevel {args.recursionLevel}")
    seqNames, speakers = findAllSeqs(args.pathDB, speaker_level=args.recursionLevel, extension=args.file_extension)     # (no sequence cache: the listing is read afresh, as before findAllSeqs had one)
    print(f"Done! Found {len(seqNames)} files and {len(speakers)} speakers!")

    nameOutput = "quantized_outputs.txt" if not args.split else f"quantized_outputs_split_{idx_split}-{num_splits}.txt"
    outputFile = os.path.join(args.pathOutput, nameOutput)
    assert not os.path.exists(outputFile), f"Output file {outputFile} already exists !!!"

    if args.split:
        startIdx, endIdx = split_bounds(len(seqNames), idx_split, num_splits)
        seqNames = seqNames[startIdx:endIdx]
        print("")
        print(f"Quantizing split {idx_split} out of {num_splits} splits, with {len(seqNames)} files "
              f"(idx in range({startIdx}, {endIdx})).")

    if args.debug:
        nsamples = 20
        print("")
        print(f"Debug mode activated, only load {nsamples} samples!")
        seqNames = seqNames[:nsamples]

    assert args.pathCheckpoint.endswith(".pt")
    clustering_args = readArgs(Path(args.pathCheckpoint).parent)
    print("")
    print(f"Clutering args:\n{json.dumps(vars(clustering_args), indent=4, sort_keys=True)}")
    print("-" * 50)
    if getattr(clustering_args, "dimReduction", None) is not None:
        raise SystemExit("the clustering run used --dimReduction, which is not supported")

    clusterModule = loadClusterModule(args.pathCheckpoint)

    print("")
    print("Loading CPC FeatureMaker")
    level_gru = getattr(clustering_args, "level_gru", None)
    updateConfig = argparse.Namespace(nLevelsGRU=level_gru) if level_gru is not None else None
    model = loadModel([clustering_args.pathCheckpoint], updateConfig=updateConfig)[0]
    if args.nobatch:
        model.gAR.keepHidden = True
    featureMaker = FeatureModule(model, clustering_args.encoder_layer)
    if not clustering_args.train_mode:
        featureMaker.eval()
    featureMaker.cuda()
    print("CPC FeatureMaker loaded!")

    print("")
    print("Quantizing audio files...")
    d = clusterModule.Ck.size(-1)
    seqQuantLines = []
    start_time = time()
    for vals in seqNames:
        file_path = os.path.join(args.pathDB, vals[1])
        cFeatures = buildFeature(featureMaker, file_path, seqNorm=False, strict=args.strict).cuda()
        nGroups = cFeatures.size(-1) // d
        units = clusterModule.assign(cFeatures.view(1, -1, d))[0].cpu().tolist()
        seqQuantLines.append(quant_line(units, nGroups))
    print(f"...done {len(seqQuantLines)} files in {time()-start_time} seconds.")

    print("")
    print(f"Saving outputs to {outputFile}")
    with open(outputFile, "w") as f:
        f.write(format_output(seqNames, seqQuantLines))


if __name__ == "__main__":
    main(sys.argv[1:])
