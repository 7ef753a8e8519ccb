"""Fit a CCA between the features of two CPC checkpoints on the same audio -- cpc/criterion/cca/train_cca.py of the reference:
its command line and defaults, its listing of the files (findAllSeqs with speaker_level=0 and the sequence cache, reread when
the cache holds another extension), CCA_info_args.json in the output directory, FeatureModule(model, onEncoder) in eval mode
for both checkpoints (keepHidden with --no_batch), buildFeature_batch or (--no_batch) buildFeature per file.

    python -m cpc2_amd.cca.train_cca --path_cp_X A/checkpoint_N.pt --path_cp_Y B/checkpoint_M.pt --path_db DB \
           --path_output OUT [--n_components 100] [--file_extension .wav] [--no_batch] [--debug]

Built differently: no frame leaves the device.  Each file's two feature sequences go through cpc2_amd.cca.Moments (count, sums
and second moments in f64, O(D^2) memory instead of every frame of both models on the host), and the fit is
cpc2_amd.cca.cca_from_moments on those moments -- sklearn's algorithm, restated (see its docstring for the one deviation, the
eigenvalue cut-off of the pseudo-inverses).

Output: cca_model_n_components_N.npz (CCAModel.save: the fitted attributes under sklearn's names and the raw moments) is the
primary file; where scikit-learn is installed the reference's cca_model_n_components_N.pkl (a pickled sklearn CCA carrying the
same attributes) is written beside it.

Deviations, each refused by name before any audio is listed:
  * --cpu is refused: there is no CPU fallback.
  * --file_extension .mp3 is refused: there is no mp3 decoder here.
  * A `level_gru` in a run's checkpoint_args.json is applied as updateConfig=Namespace(nLevelsGRU=level_gru), as eval_ABX and
    the clustering tools do (the reference passes loadModel a keyword it does not have, and stops there).
  * A file whose two feature sequences differ in length (two checkpoints with different down-sampling) is refused by name.
  * --n_components above min(frames, dimX, dimY) is refused: against the widths once both models are loaded, before any
    feature is extracted, and against the number of frames before the fit.
--strict is `type=bool` as in the reference: any non-empty value, "False" included, means True.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path


def parseArgs(argv):
    parser = argparse.ArgumentParser(description="Canonical correlation analysis between the features of two CPC checkpoints.")
    parser.add_argument("--path_cp_X", type=str, help="Checkpoint (.pt) of model X.")
    parser.add_argument("--path_cp_Y", type=str, help="Checkpoint (.pt) of model Y.")
    parser.add_argument("--path_db", type=str, help="Root directory of the audio the CCA is fitted on.")
    parser.add_argument("--path_output", type=str, help="Output directory of the CCA model.")
    parser.add_argument("--n_components", type=int, default=100, help="Number of canonical components (default: 100).")
    parser.add_argument("--file_extension", type=str, default=".wav", help="Audio file extension (default: .wav).")
    parser.add_argument("--max_size_seq", type=int, default=10240,
                        help="Samples per chunk of the batched feature extraction (default: 10240).")
    parser.add_argument("--batch_size", type=int, default=8, help="Chunks per model call (default: 8).")
    parser.add_argument("--strict", type=bool, default=True,
                        help="Every chunk has exactly max_size_seq samples (default: True; any non-empty value is True).")
    parser.add_argument("--debug", action="store_true", help="Use the first 1000 files only.")
    parser.add_argument("--no_batch", action="store_true",
                        help="One chunk per model call, the recurrent state carried from chunk to chunk.")
    parser.add_argument("--cpu", action="store_true", help="Refused: there is no CPU fallback.")
    return parser.parse_args(argv)


def refuse_unsupported(args):
    if args.cpu:
        raise SystemExit("--cpu is not supported: cpc2_amd runs only on a GPU (HIP) device. There is no CPU fallback.")
    if str(args.file_extension).lower() == ".mp3":
        raise SystemExit("--file_extension .mp3: there is no mp3 decoder in this package; decode the files to .wav or .flac first")
    for name in ("path_cp_X", "path_cp_Y"):
        path = getattr(args, name)
        if not path or not path.endswith(".pt") or not os.path.exists(path):
            raise SystemExit(f"--{name} {path}: not an existing .pt checkpoint")
    if args.n_components < 1:
        raise SystemExit(f"--n_components {args.n_components}: at least 1 is required")


def loadFeatureMakerCPC(cp_path, no_batch=False):
    from ..feature_loader import FeatureModule, getCheckpointData, loadModel
    _, _, run_args = getCheckpointData(os.path.dirname(cp_path))
    level_gru = getattr(run_args, "level_gru", None)
    updateConfig = None if level_gru is None else argparse.Namespace(nLevelsGRU=level_gru)
    model = loadModel([cp_path], updateConfig=updateConfig)[0]
    if no_batch:
        model.gAR.keepHidden = True
    feature_maker = FeatureModule(model, run_args.onEncoder)
    feature_maker.eval()
    return feature_maker


def _list_files(args):
    from ..dataset import findAllSeqs
    seqNames, _ = findAllSeqs(args.path_db, speaker_level=0, extension=args.file_extension, loadCache=True)
    if len(seqNames) == 0 or not os.path.splitext(seqNames[0][1])[1].endswith(args.file_extension):
        print("The sequence cache does not hold this extension: listing the files again")
        seqNames, _ = findAllSeqs(args.path_db, speaker_level=0, extension=args.file_extension, loadCache=False)
    return seqNames


def main(argv, timings=None):
    """timings: an optional dict that receives the seconds spent per stage (decode, features_X, features_Y, moments, solve);
    asking for it synchronises the device after every stage."""
    args = parseArgs(argv)
    refuse_unsupported(args)

    import torch

    from .. import audio
    from ..feature_loader import buildFeature_batch_device, buildFeature_device
    from . import Moments, cca_from_moments, to_sklearn

    print(f"Looking for all {args.file_extension} files in {args.path_db}")
    seqNames = _list_files(args)
    print(f"Found {len(seqNames)} files")

    Path(args.path_output).mkdir(parents=True, exist_ok=True)
    with open(os.path.join(args.path_output, "CCA_info_args.json"), "w") as file:
        json.dump(vars(args), file, indent=2)

    if args.debug:
        seqNames = seqNames[:1000]
    if len(seqNames) == 0:
        raise SystemExit("No file to fit the CCA on!")

    feature_maker_X = loadFeatureMakerCPC(args.path_cp_X, args.no_batch).cuda()
    feature_maker_Y = loadFeatureMakerCPC(args.path_cp_Y, args.no_batch).cuda()
    dim_x, dim_y = feature_maker_X.out_feature_dim, feature_maker_Y.out_feature_dim
    if args.n_components > min(dim_x, dim_y):
        raise SystemExit(f"--n_components {args.n_components} is above the narrower feature width (X: {dim_x}, Y: {dim_y})")

    def extract(feature_maker, wave):
        if args.no_batch:
            return buildFeature_device(feature_maker, wave, seqNorm=False, strict=args.strict)
        return buildFeature_batch_device(feature_maker, wave, seqNorm=False, strict=args.strict, maxSizeSeq=args.max_size_seq,
                                         batch_size=args.batch_size)

    def lap(stage, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[stage] = timings.get(stage, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    moments = Moments(dim_x, dim_y, device=next(feature_maker_X.parameters()).device)
    print("Extracting representations ...")
    start_time = time.time()
    for _, rel in seqNames:
        t = time.perf_counter()
        wave = audio.load(os.path.join(args.path_db, rel))[0]
        t = lap("decode", t)
        x_feat = extract(feature_maker_X, wave)
        t = lap("features_X", t)
        y_feat = extract(feature_maker_Y, wave)
        t = lap("features_Y", t)
        if x_feat.size(1) != y_feat.size(1):
            raise SystemExit(f"{rel}: model X gives {x_feat.size(1)} frames and model Y {y_feat.size(1)}; the two checkpoints "
                             "must have the same down-sampling")
        moments.update(x_feat, y_feat)
        lap("moments", t)
    print(f"... done {len(seqNames)} files ({moments.count} frames) in {time.time() - start_time:.2f} seconds.")

    if args.n_components > moments.count:
        raise SystemExit(f"--n_components {args.n_components} is above the number of frames ({moments.count})")
    print("Fitting CCA to the moments ...")
    t = time.perf_counter()
    model = cca_from_moments(*moments.state(), args.n_components)
    lap("solve", t)

    stem = os.path.join(args.path_output, "cca_model_n_components_%d" % args.n_components)
    model.save(stem + ".npz")
    try:
        cca = to_sklearn(model)
    except ImportError:
        print(f"scikit-learn is not installed: {stem}.pkl is not written ({stem}.npz holds the model)")
    else:
        import pickle
        with open(stem + ".pkl", "wb") as file:
            pickle.dump(cca, file)
    return model


if __name__ == "__main__":
    main(sys.argv[1:])
