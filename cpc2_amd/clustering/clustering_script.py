"""Fit k-means (or DP-means) on the features of a trained CPC model -- cpc/clustering/clustering_script.py of the
reference: same command line, same refusal of an existing output directory without --load, same files written
(args.json, training_logs.txt, checkpoint_{i}.pt, checkpoint_last.pt).

    python -m cpc2_amd.clustering.clustering_script <checkpoint.pt> <output dir> <dataset dir> -k 50 [--save]

One GPU per process: the batch is --batchSizeGPU windows (the reference multiplies it by the device count for
DataParallel).  --dimReduction and --getDistanceEstimation need the reference's criterion/research code, which is not
part of this package: they are refused before any work is done.
"""
import argparse
import json
import sys
import time
from pathlib import Path
from random import shuffle

import torch

from .clustering import fastDPMean, kMeanGPU, save_cluster_step


def parseArgs(argv):
    parser = argparse.ArgumentParser(description="Clustering module using kmeans or dpmeans.")
    parser.add_argument("pathCheckpoint", type=str, help="Path to the checkpoint of CPC module.")
    parser.add_argument("dirOutput", type=str, help="Path to the output clustering checkpoint.")
    parser.add_argument("pathDB", type=str, help="Path to the root directory containing the audio files to process")
    parser.add_argument("-k", "--nClusters", type=int, default=50, help="Number of clusters (default: 50).")
    parser.add_argument("-g", "--nGroups", type=int, default=1, help="Number of groups (default: 1).")
    parser.add_argument("-n", "--MAX_ITER", type=int, default=100, help="Number of iterations (default: 100).")
    parser.add_argument("--recursionLevel", type=int, default=2, help="Speaker level in the dataset (default: 2).")
    parser.add_argument("--extension", type=str, default=".flac", help="Audio file extension (default: .flac).")
    parser.add_argument("--seqList", type=str, default=None, help="Training sequence list (default: None).")
    parser.add_argument("--sizeWindow", type=int, default=10240, help="Window size in samples (default: 10240).")
    parser.add_argument("--debug", action="store_true", help="Use at most 1000 sequences.")
    parser.add_argument("--encoder_layer", action="store_true", help="Cluster the encoder's outputs.")
    parser.add_argument("--level_gru", type=int, default=None,
                        help="Build the model with this many recurrent layers and cluster the last (default: None).")
    parser.add_argument("--batchSizeGPU", type=int, default=50,
                        help="Windows per batch (default: 50). One GPU per process: unlike the reference, which "
                             "multiplies it by the device count for DataParallel, this is the whole batch.")
    parser.add_argument("--DPMean", action="store_true", help="DP-means instead of k-means.")
    parser.add_argument("-l", "--DPLambda", type=float, default=11, help="DP-means lambda (default: 11).")
    parser.add_argument("--perIterSize", type=int, default=-1, help="Batches per iteration (default: -1, the loader).")
    parser.add_argument("--train_mode", action="store_true", help="Keep the CPC model in train mode.")
    parser.add_argument("--dimReduction", type=str, default=None, help="Not supported here (default: None).")
    parser.add_argument("--centroidLimits", type=int, nargs=2, default=None, help="With --dimReduction only.")
    parser.add_argument("--getDistanceEstimation", action="store_true", help="Not supported here.")
    parser.add_argument("--save", action="store_true", help="Save the intermediate checkpoints in the output directory.")
    parser.add_argument("--load", type=str, help="Restart from the given clustering checkpoint")
    parser.add_argument("--save-last", type=int, default=5, help="Number of last checkpoints kept (default: 5).")
    parser.add_argument("--max-size-loaded", type=int, default=400000000,
                        help="Samples loaded at a time (default: 400000000).")
    return parser.parse_args(argv)


def refuse_unsupported(args):
    if args.dimReduction is not None:
        raise SystemExit("--dimReduction is not supported: it needs the reference's criterion/research modules, "
                         "which are out of scope for this package.")
    if args.getDistanceEstimation:
        raise SystemExit("--getDistanceEstimation is not supported: distanceEstimation is out of scope for this package.")


def main(argv):
    from ..dataset import AudioBatchData, filterSeqs, findAllSeqs
    from ..feature_loader import FeatureModule, loadModel

    args = parseArgs(argv)
    refuse_unsupported(args)
    args.pathCheckpoint = Path(args.pathCheckpoint).resolve()
    args.dirOutput = Path(args.dirOutput).resolve()
    args.pathDB = Path(args.pathDB).resolve()
    print("MAX_SIZE_LOADED is %d" % args.max_size_loaded)
    if not args.load and args.dirOutput.is_dir():
        print(f"The output directory {args.dirOutput} already exists, please check the option --load !")
        return

    seqNames, speakers = findAllSeqs(str(args.pathDB), speaker_level=args.recursionLevel, extension=args.extension)     # (no sequence cache: the listing is read afresh, as before findAllSeqs had one)
    if args.seqList is not None:
        seqNames = filterSeqs(args.seqList, seqNames)
    if args.debug:
        nsamples = 1000
        print(f"Debug mode activated, get only {nsamples} samples!")
        shuffle(seqNames)
        seqNames = seqNames[:nsamples]

    print("")
    print(f"Loading audio data at {args.pathDB}")
    start_time = time.time()
    dataset = AudioBatchData(args.pathDB, args.sizeWindow, seqNames, None, len(speakers),
                             MAX_SIZE_LOADED=args.max_size_loaded)
    print(f"Dataset loaded in {time.time()-start_time} seconds !")
    print("")

    trainLoader = dataset.getDataLoader(args.batchSizeGPU, "uniform", False, numWorkers=0)
    print(f"Length of dataLoader: {len(trainLoader)}")
    print("")

    updateConfig = None if args.level_gru is None else argparse.Namespace(nLevelsGRU=args.level_gru)
    model = loadModel([str(args.pathCheckpoint)], updateConfig=updateConfig)[0]
    featureMaker = FeatureModule(model, args.encoder_layer)
    print("Checkpoint loaded!")
    print("")
    if not args.train_mode:
        featureMaker.eval()
    featureMaker.cuda()

    args.dirOutput.mkdir(parents=True, exist_ok=True)
    with open(args.dirOutput / "args.json", "w") as file:
        json.dump({k: str(v) if isinstance(v, Path) else v for k, v in vars(args).items()}, file, indent=2)

    start_clusters = None
    if args.load is not None:
        print(f"Loading the clusters from {args.load}")
        start_clusters = torch.load(args.load, map_location="cpu")["state_dict"]["Ck"]
        print(start_clusters.size())
    print("Starting the clustering...")
    start_time = time.time()
    if args.DPMean:
        clusters = fastDPMean(trainLoader, featureMaker, args.DPLambda, MAX_ITER=args.MAX_ITER,
                              perIterSize=args.perIterSize, save_dir=args.dirOutput, save_last=args.save_last,
                              mu_start=start_clusters).cpu()
        args.nClusters = clusters.size(1)
    else:
        clusters = kMeanGPU(trainLoader, featureMaker, args.nClusters, args.nGroups, perIterSize=args.perIterSize,
                            MAX_ITER=args.MAX_ITER, save_dir=args.dirOutput, save_last=args.save_last,
                            start_clusters=start_clusters).cpu()

    print(f"Ran clustering in {time.time() - start_time:.2f} seconds")
    save_cluster_step(clusters, args.dirOutput / "checkpoint_last.pt")


if __name__ == "__main__":
    main(sys.argv[1:])
