"""Unsupervised phone segmentation of a corpus and its scores against frame-level phone labels (cpc2_amd/segmentation.py,
csrc/segment.hip).  The reference has no such tool; the command line has the shape of eval_ABX.

    python -m cpc2_amd.eval.phone_segmentation from_checkpoint CKPT PATH_DB --out DIR [--file_extension .wav] [--get_encoded]
           [--seq_norm] [--max_size_seq 64000] [--strict] [--level_gru N] [common flags]
    python -m cpc2_amd.eval.phone_segmentation from_pre_computed PATH_FEATURES --out DIR [--file_extension .pt|.npy] [common flags]

    common flags: [--pathPhone LABELS] [--pathSeqs LIST] [--pathDevSeqs LIST] [--prominence P [P ...]] [--tolerance 2]
                  [--max_length_mismatch 2] [--feature_size 0.01]

from_checkpoint loads the model with loadModel and extracts whole-utterance features with buildFeature_device: they stay on the
device until the counts are made.  The recurrent state is carried from chunk to chunk of one file (a cut every --max_size_seq
samples would otherwise look like a boundary) and reset between files.  from_pre_computed reads the [frames, dim] files that
build_zeroSpeech_features (--format npy), build_reduced_features and build_baseline_features write.

With --pathPhone (the label files of linear_separability, or the alignment_frames.txt of `common_voices_eval align`) every
threshold of --prominence (default 0.01 .. 0.30 in steps of 0.01, at most 64) is scored and the one with the best strict R-value
is chosen, the lowest among equals; with --pathDevSeqs it is chosen on the utterances of that list and the scores are reported
on the others.  An utterance whose feature and label lengths differ by more than --max_length_mismatch frames is skipped and
listed; so is one without labels.  Three files are written into --out:
    segmentation_scores.json   the arguments, per threshold the integer totals with the strict and the lenient scores, the chosen
                               threshold, and the utterances skipped, mismatched and non-finite by name
    boundaries.txt             `name t0 t1 ...` in seconds at the chosen threshold
    segmentation_log.json      the wall time of decode, model, kernels, copy and write, the device synchronised between them
Without labels exactly one --prominence is required and only boundaries.txt is written.

Refused by name before any audio is read: --file_extension .mp3, a non-empty --out, several thresholds without labels, more than 64
thresholds, --feature_size other than 0.01 with labels (the labels are one per 10 ms frame).
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

from .. import audio
from .. import segmentation as seg
from ..dataset import filterSeqs, findAllSeqs, parseSeqLabels
from ..feature_loader import FeatureModule, buildFeature_device, loadModel

STAGES = ("decode", "model", "kernels", "copy", "write")
DEFAULT_PROMINENCES = [round(0.01 * i, 2) for i in range(1, 31)]
COUNT_NAMES = ("n_hyp", "hits", "hyp_near", "ref_near")


def _common(parser):
    parser.add_argument('--pathPhone', type=str, default=None, help="Frame-level phone labels, `name l0 l1 ...` per line")
    parser.add_argument('--pathSeqs', type=str, default=None, help="List of the utterances to segment (base names)")
    parser.add_argument('--pathDevSeqs', type=str, default=None,
                        help="List of the utterances the threshold is chosen on; the scores are reported on the others")
    parser.add_argument('--prominence', type=float, nargs='+', default=None,
                        help="Prominence thresholds relative to max d - min d (default 0.01 .. 0.30)")
    parser.add_argument('--tolerance', type=int, default=2, help="Matching tolerance in frames (2 = 20 ms)")
    parser.add_argument('--max_length_mismatch', type=int, default=2,
                        help="Largest difference in frames between features and labels of a scored utterance")
    parser.add_argument('--feature_size', type=float, default=0.01, help="Size (in s) of one feature")
    parser.add_argument('--out', type=str, required=True, help="Directory the results are written into (empty or absent)")


def parse_args(argv):
    base_parser = argparse.ArgumentParser(description='Unsupervised phone segmentation')
    subparsers = base_parser.add_subparsers(dest='load')
    ckpt = subparsers.add_parser('from_checkpoint')
    ckpt.add_argument('path_checkpoint', type=str, help="Path to the model's checkpoint")
    ckpt.add_argument('path_dataset', type=str, help="Path to the dataset")
    ckpt.add_argument('--file_extension', type=str, default='.wav', help=".wav or .flac (.mp3 is refused)")
    ckpt.add_argument('--get_encoded', action='store_true', help="Segment the output of the encoder network")
    ckpt.add_argument('--seq_norm', action='store_true', help="Normalize each chunk of features across the time channel")
    ckpt.add_argument('--max_size_seq', default=64000, type=int, help="Samples per model call")
    ckpt.add_argument('--strict', action='store_true', help="Each model call takes exactly max_size_seq samples")
    ckpt.add_argument('--level_gru', type=int, default=None, help="Build the model with this many recurrent layers")
    _common(ckpt)
    pre = subparsers.add_parser('from_pre_computed')
    pre.add_argument('path_dataset', type=str, help="Path to pre-computed [frames, dim] features")
    pre.add_argument('--file_extension', type=str, default='.pt', choices=['.pt', '.npy'])
    _common(pre)
    args = base_parser.parse_args(argv)
    if args.load is None:
        base_parser.error("choose from_checkpoint or from_pre_computed")
    return args


def check_args(args):
    """The refusals, each naming its flag; nothing has been read yet."""
    if args.file_extension.lower() == ".mp3":
        raise NotImplementedError("--file_extension .mp3: there is no mp3 decoder in this package; convert the files to .wav or .flac")
    if args.prominence is None:
        if args.pathPhone is None:
            raise ValueError("--prominence: without --pathPhone there is nothing to choose a threshold by; give exactly one")
        args.prominence = list(DEFAULT_PROMINENCES)
    if len(args.prominence) > seg.MAX_THRESHOLDS:
        raise ValueError(f"--prominence: {len(args.prominence)} thresholds; at most {seg.MAX_THRESHOLDS} are supported")
    if args.pathPhone is None and len(args.prominence) != 1:
        raise ValueError(f"--prominence: {len(args.prominence)} thresholds without --pathPhone; exactly one is required")
    if args.pathPhone is None and args.pathDevSeqs is not None:
        raise ValueError("--pathDevSeqs chooses the threshold by the labels: it needs --pathPhone")
    if args.pathPhone is not None and args.feature_size != 0.01:
        raise ValueError(f"--feature_size {args.feature_size}: the labels are one per 10 ms frame; only 0.01 is scored")
    if args.feature_size <= 0:
        raise ValueError(f"--feature_size {args.feature_size} must be positive")
    if args.tolerance < 0 or args.max_length_mismatch < 0:
        raise ValueError("--tolerance and --max_length_mismatch must be >= 0")
    if os.path.exists(args.out) and (not os.path.isdir(args.out) or os.listdir(args.out)):
        raise ValueError(f"--out {args.out} exists and is not an empty directory: the tool writes its files there and overwrites "
                         "nothing")
    args.prominence = sorted(float(p) for p in args.prominence)
    return args


def _name(path):
    return os.path.basename(os.path.splitext(path)[0])


def feature_source(args, timings):
    """(names, load): load(i) -> the features [frames, dim] float32 of utterance i on the device."""
    seqs = findAllSeqs(args.path_dataset, extension=args.file_extension, loadCache=False)[0]
    seqs = sorted(seqs, key=lambda x: _name(x[1]))
    if args.pathSeqs is not None:
        seqs = filterSeqs(args.pathSeqs, seqs)
    paths = [os.path.join(args.path_dataset, x[1]) for x in seqs]
    device = torch.device("cuda")

    def lap(stage, t0):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        timings[stage] += t1 - t0
        return t1

    if args.load == 'from_checkpoint':
        update = argparse.Namespace(nLevelsGRU=args.level_gru) if args.level_gru is not None else None
        model = loadModel([args.path_checkpoint], updateConfig=update)[0]
        model.gAR.keepHidden = True
        feature_maker = FeatureModule(model, args.get_encoded).cuda().eval()

        def load(i):
            t0 = time.perf_counter()
            wave = audio.load(paths[i])[0]
            t0 = lap("decode", t0)
            if hasattr(model.gAR, "hidden"):
                model.gAR.hidden = None                    # the state streams through one file, not from file to file
            feats = buildFeature_device(feature_maker, wave, strict=args.strict, maxSizeSeq=args.max_size_seq, seqNorm=args.seq_norm)
            lap("model", t0)
            return feats[0].float().contiguous()
    else:
        def load(i):
            t0 = time.perf_counter()
            if args.file_extension == '.npy':
                feats = torch.from_numpy(np.load(paths[i]))
            else:
                feats = torch.load(paths[i], 'cpu')
            if feats.dim() == 3 and feats.size(0) == 1:
                feats = feats[0]
            if feats.dim() != 2:
                raise ValueError(f"{paths[i]}: expected [frames, dim] features, got {tuple(feats.shape)}")
            t0 = lap("decode", t0)
            feats = feats.float().contiguous().to(device)
            lap("copy", t0)
            return feats

    return [_name(p) for p in paths], load


def totals_and_scores(counts, n_ref, rows):
    """Per threshold: the integer totals over the utterances `rows` and the strict and lenient scores made from them."""
    out = []
    sub = counts[rows].sum(axis=0, dtype=np.int64) if len(rows) else np.zeros(counts.shape[1:], np.int64)
    total_ref = int(n_ref[rows].sum()) if len(rows) else 0
    for k in range(counts.shape[1]):
        n_hyp, hits, hyp_near, ref_near = (int(v) for v in sub[k])
        out.append({"n_ref": total_ref, "n_hyp": n_hyp, "hits": hits, "hyp_near": hyp_near, "ref_near": ref_near,
                    "strict": seg.boundary_scores(total_ref, n_hyp, hits),
                    "lenient": seg.boundary_scores(total_ref, n_hyp, hyp_near, ref_hits=ref_near)})
    return out


def choose(per_threshold):
    """The index of the best strict R-value; the lowest threshold among equals (the thresholds are sorted)."""
    best = 0
    for k, row in enumerate(per_threshold):
        if row["strict"]["rval"] > per_threshold[best]["strict"]["rval"]:
            best = k
    return best


def main(argv):
    args = check_args(parse_args(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available: phone_segmentation makes the "
                           "dissimilarity, the peaks and the counts on the device. There is no CPU fallback.")
    labels = parseSeqLabels(args.pathPhone)[0] if args.pathPhone is not None else None
    dev_names = None
    if args.pathDevSeqs is not None:
        with open(args.pathDevSeqs) as f:
            dev_names = {line.strip() for line in f if line.strip()}
    timings = {stage: 0.0 for stage in STAGES}
    names, load = feature_source(args, timings)
    if not names:
        raise ValueError(f"no {args.file_extension} file found under {args.path_dataset}")

    kept, pieces, lengths, refs, limits, statuses = [], [], [], [], [], []
    skipped, mismatched = [], []
    for i, name in enumerate(names):
        if labels is not None and name not in labels:
            skipped.append(name)
            continue
        feats = load(i)
        n_frames = feats.size(0)
        if labels is not None:
            lab = labels[name]
            if abs(n_frames - len(lab)) > args.max_length_mismatch:
                mismatched.append({"name": name, "frames": n_frames, "labels": len(lab)})
                continue
            n_l = min(n_frames, len(lab))
            refs.append(seg.reference_boundaries(lab, n_l))
            limits.append(n_l)
        t0 = time.perf_counter()
        d, status = seg.frame_dissimilarity(feats, return_status=True)
        pieces.append(torch.cat([d, d.new_full((min(n_frames, 1),), float("nan"))]))      # one slot per frame: the packed layout
        statuses.append(status)
        torch.cuda.synchronize()
        timings["kernels"] += time.perf_counter() - t0
        kept.append(name)
        lengths.append(n_frames)
    if not kept:
        raise ValueError("no utterance left to segment: every one was skipped (no labels) or mismatched")

    t0 = time.perf_counter()
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64)
    result = seg.find_boundaries(torch.cat(pieces), offsets, lengths, args.prominence, ref=refs if labels is not None else None,
                                 tol=args.tolerance, limits=limits if labels is not None else None)
    torch.cuda.synchronize()
    timings["kernels"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    counts = result.counts.cpu().numpy()
    status = np.maximum(torch.cat(statuses).cpu().numpy(), result.status.cpu().numpy())
    timings["copy"] += time.perf_counter() - t0
    non_finite = [n for n, s in zip(kept, status) if s != 0]

    scores = None
    chosen = 0
    if labels is not None:
        n_ref = np.array([len(r) for r in refs], dtype=np.int64)
        ok = np.array([s == 0 for s in status])
        is_dev = np.array([dev_names is not None and n in dev_names for n in kept])
        select_rows = np.flatnonzero(ok & is_dev) if dev_names is not None else np.flatnonzero(ok)
        report_rows = np.flatnonzero(ok & ~is_dev)
        if n_ref[select_rows].sum() == 0 or n_ref[report_rows].sum() == 0:
            raise ValueError("no reference boundary among the utterances the threshold is chosen on, or among those reported: "
                             "the scores are undefined")
        selection = totals_and_scores(counts, n_ref, select_rows)
        chosen = choose(selection)
        report = totals_and_scores(counts, n_ref, report_rows)
        scores = {"args": vars(args), "prominence": args.prominence, "chosen_index": chosen,
                  "chosen_prominence": args.prominence[chosen], "chosen_on": "dev" if dev_names is not None else "all",
                  "n_utterances": int(len(report_rows)), "per_threshold": report,
                  "dev_per_threshold": selection if dev_names is not None else None,
                  "dev_utterances": [kept[r] for r in select_rows] if dev_names is not None else None,
                  "scores": report[chosen], "skipped": skipped, "mismatched": mismatched, "non_finite": non_finite}

    t0 = time.perf_counter()
    frames = seg.select_boundaries(result, args.prominence[chosen], limits if labels is not None else None)
    timings["copy"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "boundaries.txt", "w") as f:
        for name, fr in zip(kept, frames):
            f.write(" ".join([name] + [format_time(int(q), args.feature_size) for q in fr]) + "\n")
    if scores is not None:
        with open(out_dir / "segmentation_scores.json", "w") as f:
            json.dump(scores, f, indent=2)
    timings["write"] += time.perf_counter() - t0
    if scores is not None:
        with open(out_dir / "segmentation_log.json", "w") as f:
            json.dump({"utterances": len(kept), "frames": int(sum(lengths)), "seconds": timings}, f, indent=2)
        best = scores["scores"]["strict"]
        print(f"prominence {args.prominence[chosen]}: P {best['precision']:.4f} R {best['recall']:.4f} F1 {best['f1']:.4f} "
              f"OS {best['os']:.4f} R-value {best['rval']:.4f} on {len(report_rows)} utterances")
    print(f"{len(kept)} utterances: " + ", ".join(f"{stage} {timings[stage]:.3f} s" for stage in STAGES))
    return {"scores": scores, "names": kept, "boundaries": frames, "timings": timings}


def format_time(frame, feature_size=0.01):
    """Frame q as seconds: q * 160 / 16000 at the 10 ms frame of the encoder, else q * feature_size."""
    return f"{frame * 160 / 16000:.2f}" if feature_size == 0.01 else repr(frame * feature_size)


if __name__ == "__main__":
    main(sys.argv[1:])
