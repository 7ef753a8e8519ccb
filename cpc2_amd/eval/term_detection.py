"""Query-by-example spoken term detection of a trained CPC model or of pre-computed features (cpc2_amd/term_detection.py,
csrc/sdtw.hip).  The reference has no such tool; the command line has the shape of eval_ABX.

    python -m cpc2_amd.eval.term_detection from_checkpoint CKPT DOC_DIR --queries Q.txt --relevance R.txt --out DIR [flags]
    python -m cpc2_amd.eval.term_detection from_pre_computed FEATURE_DIR --queries Q.txt --relevance R.txt --out DIR [flags]
    python -m cpc2_amd.eval.term_detection from_units QUANTIZED.txt --queries Q.txt --relevance R.txt --out DIR
           [--query_units QUANTIZED_Q.txt] [--doc_list L] [--distance_mode cosine|euclidian] [--top 100] [--feature_size 0.01]
           [--max_doc_frames N]

    flags: [--query_dir D] [--doc_list L] [--file_extension .flac|.wav|.npy|.pt] [--distance_mode cosine|euclidian]
           [--feature_size 0.01] [--top 100] [--seqNorm] [--max_doc_frames N]

Q.txt has lines `query_id file_stem [onset_s offset_s]`: a query is a whole file or a span of one, cut on the feature grid
(frames max(0, ceil(onset / feature_size - 0.5)) up to min(frames, floor(offset / feature_size - 0.5)), the rule of the ABX item
files).  The file is looked up in --query_dir when given, else among the documents.  R.txt has lines
`query_id doc_stem [onset_s offset_s]`: the document contains the term; the span optionally says where.  Every file under
DOC_DIR / FEATURE_DIR with the extension is a document (--doc_list: only the base names it lists).

Every query is scored against every document with the subsequence DTW of cpc_sdtw and the documents are ranked per query
(ascending score, ties by document order, NaN last).  A query cut from a document is never scored against that document: the
pair is excluded, not counted as a miss.  Cosine mode normalises the rows with normalize_with_singularity, as ABX does.  Files
with non-finite features, empty queries and documents longer than --max_doc_frames (default: what the package sizes the kernel's
scratch for, MAX_DOC_FRAMES = 16384) are left out and listed by name.  Three files are written into --out:
    term_detection_scores.json   MAP, mean P@10, mean P@N and MRR over the queries with a relevant candidate, the query counts, the
                                 arguments, the lists above and, where R.txt gives spans, the share of relevant pairs whose
                                 detected span overlaps a labelled one with IoU >= 0.5
    detections.txt               the top --top documents per query: `query doc rank score start_s end_s relevant`
    term_detection_log.json      the wall time of decode, model, copy, kernels, rank and write, the device synchronised between them

from_units searches QUANTIZED units (csrc/sdtw_units.hip): QUANTIZED.txt is the quantized_outputs.txt that
clustering_quantization and segment_quantization write (or the directory that holds one), read by unit_quality.read_quantized: a
document is a line of it, a query a line (of --query_units when given) or a span of one.  The frame distance is then one of two
numbers, those the chosen --distance_mode gives on one-hot rows (abx_group_computation.unit_frame_distances: 0 and 0.5 for
cosine, 0 and sqrt 2 for euclidian), and cpc_sdtw_units runs the same recurrence on the unit ids.  Ranks, scores and files are
made by the same code; the log also names the source, the number of distinct units and the two distances.  --seqNorm and
--query_dir are refused with from_units (there is no feature to normalise and no file to look up).

Refused by name before any audio or feature file is opened: --file_extension .mp3, a non-empty --out, a Q.txt or R.txt that is
missing or has malformed lines, a query_id in R.txt that Q.txt lacks, a non-positive --feature_size, --top < 1.
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

from .. import audio
from .. import term_detection as td
from ..dataset import filterSeqs, findAllSeqs
from ..feature_loader import FeatureModule, buildFeature_device, loadModel, seqNormalization
from .ABX import abx_group_computation as abx_g
from .ABX.abx_iterators import normalize_with_singularity
from .unit_quality import read_quantized

STAGES = ("decode", "model", "copy", "kernels", "rank", "write")
MAX_DOC_FRAMES = 16384             # documents the scratch is sized for by default: 24 bytes x frames per workgroup


def _common(parser):
    parser.add_argument('--queries', type=str, required=True, help="`query_id file_stem [onset_s offset_s]` per line")
    parser.add_argument('--relevance', type=str, required=True, help="`query_id doc_stem [onset_s offset_s]` per line")
    parser.add_argument('--out', type=str, required=True, help="Directory the results are written into (empty or absent)")
    parser.add_argument('--query_dir', type=str, default=None, help="Where the queries' files are (default: the documents)")
    parser.add_argument('--doc_list', type=str, default=None, help="List of the documents to search (base names)")
    parser.add_argument('--distance_mode', type=str, default='cosine', choices=['cosine', 'euclidian'])
    parser.add_argument('--feature_size', type=float, default=0.01, help="Size (in s) of one feature")
    parser.add_argument('--top', type=int, default=100, help="Documents listed per query in detections.txt")
    parser.add_argument('--seqNorm', action='store_true', help="Normalize each file's features across the time channel")
    parser.add_argument('--max_doc_frames', type=int, default=MAX_DOC_FRAMES, help="Longer documents are left out and listed")


def parse_args(argv):
    base_parser = argparse.ArgumentParser(description='Query-by-example spoken term detection')
    subparsers = base_parser.add_subparsers(dest='load')
    ckpt = subparsers.add_parser('from_checkpoint')
    ckpt.add_argument('path_checkpoint', type=str, help="Path to the model's checkpoint")
    ckpt.add_argument('path_dataset', type=str, help="Path to the documents")
    ckpt.add_argument('--file_extension', type=str, default='.wav', help=".wav or .flac (.mp3 is refused)")
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
    units.add_argument('--query_units', type=str, default=None, help="The queries' quantized_outputs.txt (default: the documents)")
    _common(units)
    args = base_parser.parse_args(argv)
    if args.load is None:
        base_parser.error("choose from_checkpoint, from_pre_computed or from_units")
    return args


def units_file(path, flag="from_units"):
    """The unit file behind `path`: the file itself, or the quantized_outputs.txt of a directory (the per-penalty layout of
    segment_quantization)."""
    if os.path.isdir(path):
        path = os.path.join(path, "quantized_outputs.txt")
    if not os.path.isfile(path):
        raise ValueError(f"{flag} {path}: no such unit file")
    return path


def _read_spans(path, flag, what):
    """The lines `id stem [onset offset]` of a Q.txt / R.txt: [(id, stem, onset or None, offset or None)]."""
    if not os.path.isfile(path):
        raise ValueError(f"{flag} {path}: no such file")
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            if len(fields) not in (2, 4):
                raise ValueError(f"{flag} {path}:{no}: expected `{what} [onset_s offset_s]`, got {len(fields)} fields")
            onset = offset = None
            if len(fields) == 4:
                try:
                    onset, offset = float(fields[2]), float(fields[3])
                except ValueError:
                    raise ValueError(f"{flag} {path}:{no}: onset / offset are not numbers: {fields[2]!r} {fields[3]!r}") from None
                if not (math.isfinite(onset) and math.isfinite(offset) and 0 <= onset < offset):
                    raise ValueError(f"{flag} {path}:{no}: needs 0 <= onset < offset, got {onset} {offset}")
            rows.append((fields[0], fields[1], onset, offset))
    return rows


def check_args(args):
    """The refusals, each naming its flag; no audio or feature file has been opened.  Leaves the parsed Q.txt / R.txt in
    args.query_rows / args.relevance_rows."""
    if args.load == 'from_units':
        if args.seqNorm:
            raise ValueError("--seqNorm with from_units: units are not features, there is nothing to normalise")
        if args.query_dir is not None:
            raise ValueError("--query_dir with from_units: the queries' units come from --query_units")
    else:
        ext = args.file_extension.lower()
        if ext == ".mp3":
            raise NotImplementedError("--file_extension .mp3: there is no mp3 decoder in this package; convert the files to .wav or .flac")
        allowed = (".wav", ".flac") if args.load == 'from_checkpoint' else (".pt", ".npy")
        if ext not in allowed:
            raise ValueError(f"--file_extension {args.file_extension}: {args.load} reads {' or '.join(allowed)}")
    if not args.feature_size > 0 or not math.isfinite(args.feature_size):
        raise ValueError(f"--feature_size {args.feature_size} must be positive")
    if args.top < 1:
        raise ValueError(f"--top {args.top} must be >= 1")
    if args.max_doc_frames < 1:
        raise ValueError(f"--max_doc_frames {args.max_doc_frames} must be >= 1")
    if os.path.exists(args.out) and (not os.path.isdir(args.out) or os.listdir(args.out)):
        raise ValueError(f"--out {args.out} exists and is not an empty directory: the tool writes its files there and overwrites "
                         "nothing")
    queries = _read_spans(args.queries, "--queries", "query_id file_stem")
    if not queries:
        raise ValueError(f"--queries {args.queries}: no query")
    ids = [q[0] for q in queries]
    if len(set(ids)) != len(ids):
        dup = sorted({i for i in ids if ids.count(i) > 1})
        raise ValueError(f"--queries {args.queries}: query_id given twice: {' '.join(dup)}")
    relevance = _read_spans(args.relevance, "--relevance", "query_id doc_stem")
    unknown = sorted({r[0] for r in relevance} - set(ids))
    if unknown:
        raise ValueError(f"--relevance {args.relevance}: query_id not in --queries: {' '.join(unknown)}")
    args.query_rows, args.relevance_rows = queries, relevance
    if args.load == 'from_units':
        args.path_units = units_file(args.path_units)
        if args.query_units is not None:
            args.query_units = units_file(args.query_units, "--query_units")
    return args


def _name(path):
    return os.path.basename(os.path.splitext(path)[0])


def _listing(root, extension, keep=None):
    seqs = findAllSeqs(root, extension=extension, loadCache=False)[0]
    seqs = sorted(seqs, key=lambda x: _name(x[1]))
    if keep is not None:
        seqs = filterSeqs(keep, seqs)
    return {_name(x[1]): os.path.join(root, x[1]) for x in seqs}


def span_frames(onset, offset, n_frames, feature_size):
    """Frames [first, last) of a span in seconds on the feature grid: the rule of the ABX item files."""
    step = 1 / feature_size
    first = max(0, int(math.ceil(step * onset - 0.5)))
    last = min(n_frames, int(math.floor(step * offset - 0.5)))
    return first, last


def feature_loader(args, timings):
    """load(path) -> the features [frames, dim] float32 of one file on the device."""
    device = torch.device("cuda")

    def lap(stage, t0):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        timings[stage] += t1 - t0
        return t1

    if args.load == 'from_checkpoint':
        model = loadModel([args.path_checkpoint])[0]
        model.gAR.keepHidden = True
        feature_maker = FeatureModule(model, args.get_encoded).cuda().eval()

        def load(path):
            t0 = time.perf_counter()
            wave = audio.load(path)[0]
            t0 = lap("decode", t0)
            if hasattr(model.gAR, "hidden"):
                model.gAR.hidden = None                    # the state streams through one file, not from file to file
            feats = buildFeature_device(feature_maker, wave, strict=args.strict, maxSizeSeq=args.max_size_seq, seqNorm=args.seqNorm)
            lap("model", t0)
            return feats[0].float().contiguous()
    else:
        def load(path):
            t0 = time.perf_counter()
            feats = torch.from_numpy(np.load(path)) if args.file_extension == '.npy' else torch.load(path, 'cpu')
            if feats.dim() == 3 and feats.size(0) == 1:
                feats = feats[0]
            if feats.dim() != 2:
                raise ValueError(f"{path}: expected [frames, dim] features, got {tuple(feats.shape)}")
            t0 = lap("decode", t0)
            feats = feats.float().contiguous().to(device)
            if args.seqNorm and feats.size(0) > 1:
                feats = seqNormalization(feats.unsqueeze(0))[0].contiguous()
            lap("copy", t0)
            return feats

    return load


def unit_distances(distance_mode):
    """(d_same, d_diff) of --distance_mode on one-hot rows: what the feature sources would compute on the one-hot expansion of the
    units (cosine mode normalises the rows, euclidian does not)."""
    cosine = distance_mode == 'cosine'
    return abx_g.unit_frame_distances(2, cosine, abx_g.get_cosine_distance_batch if cosine else abx_g.get_euclidian_distance_batch)


def read_units(path, flag):
    """unit_quality.read_quantized, with a unit id that does not fit the kernels' int32 refused by the file's name."""
    try:
        return read_quantized(path)
    except OverflowError as err:
        raise ValueError(f"{flag} {path}: a unit id does not fit int32 ({err})") from None


def unit_listing(args, timings):
    """from_units: (doc_paths, query_paths, load) in the shapes main uses for files.  A "path" is (file, name), so that a query
    taken from the documents' own file is the document it is excluded from, and load(path) gives the line's units."""
    t0 = time.perf_counter()
    store = {("doc", name): units for name, units in read_units(args.path_units, "from_units")}
    doc_names = sorted(name for _, name in store)
    if args.doc_list is not None:
        with open(args.doc_list, 'r') as f:
            wanted = {p.strip() for p in f.readlines() if p.strip()}
        doc_names = [name for name in doc_names if name in wanted]
    doc_paths = {name: ("doc", name) for name in doc_names}
    if args.query_units is not None:
        queries = {("query", name): units for name, units in read_units(args.query_units, "--query_units")}
        query_paths = {key[1]: key for key in queries}
        store.update(queries)
    else:
        query_paths = doc_paths
    timings["decode"] += time.perf_counter() - t0
    return doc_paths, query_paths, store.__getitem__


def iou(a0, a1, b0, b1):
    inter = max(0.0, min(a1, b1) - max(a0, b0))
    union = max(a1, b1) - min(a0, b0)
    return inter / union if union > 0 else 0.0


def format_time(frame, feature_size=0.01):
    """Frame q as seconds: q * 160 / 16000 at the 10 ms frame of the encoder, else q * feature_size."""
    return f"{frame * 160 / 16000:.2f}" if feature_size == 0.01 else repr(frame * feature_size)


def main(argv):
    args = check_args(parse_args(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("cpc2_amd runs only on a GPU (HIP) device and none is available: term_detection makes the frame "
                           "distances and the subsequence DTW on the device. There is no CPU fallback.")
    timings = {stage: 0.0 for stage in STAGES}
    from_units = args.load == 'from_units'
    if from_units:
        # a "path" is (which file, name) and its "features" are the line's unit ids (int32 numpy)
        doc_paths, query_paths, load = unit_listing(args, timings)
        if not doc_paths:
            raise ValueError(f"from_units {args.path_units}: no document" + (" named in --doc_list" if args.doc_list else ""))
    else:
        doc_paths = _listing(args.path_dataset, args.file_extension, args.doc_list)
        if not doc_paths:
            raise ValueError(f"no {args.file_extension} document found under {args.path_dataset}")
        query_paths = _listing(args.query_dir, args.file_extension) if args.query_dir is not None else doc_paths
        load = feature_loader(args, timings)
    missing_queries = [q[0] for q in args.query_rows if q[1] not in query_paths]
    cosine = args.distance_mode == 'cosine'

    # ---- features: every file once; items are spans of one frames buffer ----
    pieces, file_span, n_rows, dim = [], {}, 0, None
    non_finite, too_long = [], []

    def add_file(path):
        """(first row, frames) of a file in the buffer, or None when it is left out."""
        nonlocal n_rows, dim
        if path in file_span:
            return file_span[path]
        feats = load(path)
        if not from_units:
            if dim is None:
                dim = feats.size(1)
            if feats.size(1) != dim:
                raise ValueError(f"{path}: {feats.size(1)} feature columns, the files before it have {dim}")
            if not bool(torch.isfinite(feats).all()):
                non_finite.append(_name(path))
                file_span[path] = None
                return None
            if cosine and feats.size(0):
                feats = normalize_with_singularity(feats)
        file_span[path] = (n_rows, len(feats))
        pieces.append(feats)
        n_rows += len(feats)
        return file_span[path]

    offs, lens, doc_names = [], [], []
    for name, path in doc_paths.items():
        span = add_file(path)
        if span is None or span[1] < 1:
            continue
        if span[1] > args.max_doc_frames:
            too_long.append(name)
            continue
        doc_names.append(name)
        offs.append(span[0])
        lens.append(span[1])
    n_docs = len(doc_names)
    if n_docs == 0:
        raise ValueError("no document left to search: every one was empty, non-finite or longer than --max_doc_frames")
    doc_index = {name: i for i, name in enumerate(doc_names)}
    query_ids, query_items, exclude, empty_queries = [], [], [], []
    for qid, stem, onset, offset in args.query_rows:
        if stem not in query_paths:
            continue
        span = add_file(query_paths[stem])
        if span is None:
            continue
        first, last = (0, span[1]) if onset is None else span_frames(onset, offset, span[1], args.feature_size)
        if last - first < 1:
            empty_queries.append(qid)
            continue
        item = len(offs)
        offs.append(span[0] + first)
        lens.append(last - first)
        query_ids.append(qid)
        query_items.append(item)
        if stem in doc_index and doc_paths[stem] == query_paths[stem]:
            exclude.append((item, doc_index[stem]))                    # never scored against the document it was cut from
    if not query_ids:
        raise ValueError("no query left: every one was missing, empty or non-finite")

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

    t0 = time.perf_counter()
    if from_units:
        score, span, pair_q, pair_doc = td.subsequence_dtw_units(frames, item_off, item_len, query_items, np.arange(n_docs),
                                                                 source_log["d_same"], source_log["d_diff"], exclude=exclude,
                                                                 lens_host=lens)
    else:
        score, span, pair_q, pair_doc = td.subsequence_dtw(frames, item_off, item_len, query_items, np.arange(n_docs),
                                                           args.distance_mode, exclude=exclude, lens_host=lens)
    torch.cuda.synchronize()
    timings["kernels"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    order, ranks = td.rank(score, pair_q, pair_doc)
    torch.cuda.synchronize()
    timings["rank"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    score_h, span_h = score.cpu().numpy(), span.cpu().numpy()
    timings["copy"] += time.perf_counter() - t0

    # ---- relevance, scores ----
    q_pos = {qid: k for k, qid in enumerate(query_ids)}
    labelled, relevant_missing = {}, []
    for qid, stem, onset, offset in args.relevance_rows:
        if qid not in q_pos:
            continue
        if stem not in doc_index:
            relevant_missing.append(f"{qid} {stem}")
            continue
        labelled.setdefault((q_pos[qid], doc_index[stem]), [])
        if onset is not None:
            labelled[(q_pos[qid], doc_index[stem])].append((onset, offset))
    relevant = np.fromiter(((int(q), int(d)) in labelled for q, d in zip(pair_q, pair_doc)), dtype=bool, count=len(pair_q))
    result = td.metrics(ranks, pair_q, relevant, len(query_ids), names=query_ids)
    n_with_span = n_overlap = 0
    for p in np.flatnonzero(relevant):
        spans = labelled[(int(pair_q[p]), int(pair_doc[p]))]
        if not spans or span_h[p, 0] < 0:
            continue
        n_with_span += 1
        d0, d1 = span_h[p, 0] * args.feature_size, (span_h[p, 1] + 1) * args.feature_size
        n_overlap += max(iou(d0, d1, a, b) for a, b in spans) >= 0.5
    per_query = result.pop("per_query")
    scores = {"map": result["map"], "p_at_10": result["p_at_10"], "p_at_n": result["p_at_n"], "mrr": result["mrr"],
              "n_queries": len(args.query_rows), "n_queries_searched": len(query_ids), "n_queries_scored": result["n_scored"],
              "n_queries_without_relevant": result["n_without_relevant"], "queries_without_relevant": result["without_relevant"],
              "n_documents": n_docs, "n_pairs": int(len(pair_q)), "n_excluded_pairs": len(exclude),
              "span_iou_at_0.5": (n_overlap / n_with_span) if n_with_span else None, "n_relevant_pairs_with_span": n_with_span,
              "per_query": per_query, "missing_queries": missing_queries, "empty_queries": empty_queries, "non_finite": non_finite,
              "too_long": too_long, "relevant_missing": relevant_missing,
              "args": {k: v for k, v in vars(args).items() if k not in ("query_rows", "relevance_rows")}}

    t0 = time.perf_counter()
    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "detections.txt", "w") as f:
        for p in order:
            if ranks[p] > args.top:
                continue
            start, end = int(span_h[p, 0]), int(span_h[p, 1])
            times = ("nan", "nan") if start < 0 else (format_time(start, args.feature_size), format_time(end + 1, args.feature_size))
            f.write(f"{query_ids[pair_q[p]]} {doc_names[pair_doc[p]]} {ranks[p]} {float(score_h[p]):.8g} {times[0]} {times[1]} "
                    f"{int(relevant[p])}\n")
    with open(out_dir / "term_detection_scores.json", "w") as f:
        json.dump(scores, f, indent=2)
    timings["write"] += time.perf_counter() - t0
    cells = int((np.asarray(lens, dtype=np.int64)[np.asarray(query_items)[pair_q]] * np.asarray(lens, dtype=np.int64)[pair_doc]).sum())
    with open(out_dir / "term_detection_log.json", "w") as f:
        json.dump({"documents": n_docs, "queries": len(query_ids), "pairs": int(len(pair_q)), "cells": cells, "frames": int(n_rows),
                   "feature_columns": int(dp), **source_log, "seconds": timings}, f, indent=2)
    print(f"MAP {scores['map']:.4f} P@10 {scores['p_at_10']:.4f} P@N {scores['p_at_n']:.4f} MRR {scores['mrr']:.4f} over "
          f"{result['n_scored']} of {len(query_ids)} queries, {n_docs} documents")
    print(f"{len(pair_q)} pairs: " + ", ".join(f"{stage} {timings[stage]:.3f} s" for stage in STAGES))
    return {"scores": scores, "query_ids": query_ids, "doc_names": doc_names, "score": score_h, "span": span_h, "pair_q": pair_q,
            "pair_doc": pair_doc, "ranks": ranks, "order": order, "relevant": relevant, "timings": timings}


if __name__ == "__main__":
    main(sys.argv[1:])
