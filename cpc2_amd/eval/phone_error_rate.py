"""Phone error rate of a CTC probe: scores the run directory that
`python -m cpc2_amd.eval.linear_separability ... --pathPhone LABELS --CTC --pathCheckpoint PROBE_DIR` wrote.

    python -m cpc2_amd.eval.phone_error_rate PROBE_DIR [--pathVal F] [--pathDB D] [--pathPhone F] [--nKeep 100]
                                                       [--batchSizeGPU B] [--debug] [--out FILE.json]

PROBE_DIR/checkpoint_args.json gives pathDB, pathVal, pathPhone, load, get_encoded, size_window, file_extension and batchSizeGPU;
the newest PROBE_DIR/checkpoint_N.pt gives the feature maker's state (gEncoder) and the classifier's (cpcCriterion).  The model
and the CTCPhoneCriterion are rebuilt, the validation windows are read as linear_separability reads them (sequential, no
shuffling), and every window's softmax(criterion.getPrediction(c)) goes through the CTC prefix beam search (nKeep prefixes; the
best one is the hypothesis) and the alignment score against the window's collapsed frame labels (cpc2_amd/seq_alignment.py:
getPER of the reference, cpc/criterion/seq_alignment.py).  Prints the mean and the standard deviation over windows in the words
of the reference's cpc/eval/common_voices_eval.py.  A run that was not trained with --CTC is refused before any audio is read.
"""
import argparse
import json
import os
import sys
import time

import torch

from .. import criterion as cr
from .. import feature_loader as fl
from ..dataset import AudioBatchData, filterSeqs, findAllSeqs, parseSeqLabels
from ..seq_alignment import mean_std, window_PER


def parse_args(argv):
    parser = argparse.ArgumentParser(description="Phone error rate of a CTC probe trained by linear_separability --CTC")
    parser.add_argument('pathProbe', type=str, help="Run directory written by linear_separability --pathPhone ... --CTC.")
    parser.add_argument('--pathVal', type=str, default=None, help="List of the sequences to score (default: the run's).")
    parser.add_argument('--pathDB', type=str, default=None, help="Directory of the audio data (default: the run's).")
    parser.add_argument('--pathPhone', type=str, default=None, help="Phone labels (default: the run's).")
    parser.add_argument('--nKeep', type=int, default=100, help="Beam width of the CTC prefix search.")
    parser.add_argument('--batchSizeGPU', type=int, default=None, help="Windows per batch (default: the run's).")
    parser.add_argument('--debug', action='store_true', help="Score the first 100 sequences only.")
    parser.add_argument('--out', type=str, default=None, help="Write mean, standard deviation, windows, nKeep and ties as JSON.")
    return parser.parse_args(argv)


def _checkpoint_index(name):
    stem, ext = os.path.splitext(name)
    return int(stem[11:]) if ext == ".pt" and stem.startswith("checkpoint_") and stem[11:].isdigit() else None


def load_run(path_probe, overrides):
    """(run arguments with the overrides applied, path of the newest checkpoint) of a probe directory; refuses by name what is
    not a CTC probe.  Reads two small files, no audio."""
    path_args = os.path.join(path_probe, "checkpoint_args.json")
    if not os.path.isfile(path_args):
        raise SystemExit(f"{path_probe}: no checkpoint_args.json -- not a run directory of cpc2_amd.eval.linear_separability")
    with open(path_args) as f:
        run = argparse.Namespace(**json.load(f))
    if getattr(run, "pathPhone", None) is None or not getattr(run, "CTC", False):
        raise SystemExit(f"{path_probe}: this run was not trained with --pathPhone ... --CTC (pathPhone={getattr(run, 'pathPhone', None)}, "
                         f"CTC={getattr(run, 'CTC', False)}): the phone error rate is defined for the CTC probe only.")
    if getattr(run, "get_encoded", False):
        raise SystemExit(f"{path_probe}: --get_encoded with --CTC is not implemented (linear_separability refuses it too).")
    for key in ("pathVal", "pathDB", "pathPhone", "batchSizeGPU"):
        if getattr(overrides, key) is not None:
            setattr(run, key, getattr(overrides, key))
    numbered = [(idx, name) for name in os.listdir(path_probe) for idx in [_checkpoint_index(name)] if idx is not None]
    if not numbered:
        raise SystemExit(f"{path_probe}: no checkpoint_N.pt")
    return run, os.path.join(path_probe, max(numbered)[1])


class _Probabilities:
    """featureMaker of getPER: a batch of the loader -> softmax over the classes of the probe's predictions, [N, S, P]."""

    def __init__(self, model, criterion, times):
        self.model, self.criterion, self.times = model, criterion, times

    def _lap(self, stage, t0):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.times[stage] = self.times.get(stage, 0.0) + now - t0
        return now

    def __call__(self, data):
        t0 = self._lap("search_and_score", self.times.pop("_mark", time.perf_counter()))
        c_feature, _, _ = self.model(data[0][:, 0], None)
        t0 = self._lap("features", t0)
        probs = torch.softmax(self.criterion.getPrediction(c_feature), dim=2)
        self.times["_mark"] = self._lap("probe", t0)
        return probs


def main(argv):
    args = parse_args(argv)
    run, path_checkpoint = load_run(args.pathProbe, args)
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available. There is no CPU fallback.")
    if len(run.load) != 1:
        raise SystemExit(f"{len(run.load)} checkpoints in the run's `load`: exactly one is supported.")

    t_start = time.perf_counter()
    seq_names, speakers = findAllSeqs(run.pathDB, extension=run.file_extension)
    phone_labels, n_phones = parseSeqLabels(run.pathPhone)
    state = torch.load(path_checkpoint, "cpu")
    model, hidden_gar, _ = fl.loadModel(run.load, loadStateDict=False)
    model.load_state_dict(state["gEncoder"], strict=False)
    criterion = cr.CTCPhoneCriterion(hidden_gar, n_phones, False)
    criterion.load_state_dict(state["cpcCriterion"])
    model.cuda().eval()
    criterion.cuda().eval()
    model.optimize = False

    seq_val = filterSeqs(run.pathVal, seq_names)
    if args.debug:
        seq_val = seq_val[:100]
    db_val = AudioBatchData(run.pathDB, run.size_window, seq_val, phone_labels, len(speakers))
    val_loader = db_val.getDataLoader(run.batchSizeGPU, 'sequential', False, numWorkers=0)
    torch.cuda.synchronize()
    times = {"load": time.perf_counter() - t_start, "_mark": time.perf_counter()}

    pers, tied = window_PER(val_loader, _Probabilities(model, criterion, times), criterion.BLANK_LABEL, args.nKeep)
    torch.cuda.synchronize()
    times["search_and_score"] = times.get("search_and_score", 0.0) + time.perf_counter() - times.pop("_mark")
    if len(pers) == 0:
        raise SystemExit(f"{run.pathVal}: no window to score")
    mean, std = mean_std(pers)
    print(f"Average PER {mean}")
    print(f"Standard deviation PER {std}")
    if args.out is not None:
        with open(args.out, 'w') as f:
            json.dump(dict(mean=mean, std=std, windows=int(len(pers)), nKeep=args.nKeep, tied_windows=int(tied.sum()),
                           checkpoint=os.path.abspath(path_checkpoint), seconds={k: round(v, 6) for k, v in times.items()}),
                      f, indent=2)
    return mean


if __name__ == "__main__":
    main(sys.argv[1:])
