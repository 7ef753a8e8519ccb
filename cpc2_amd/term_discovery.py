"""Unsupervised spoken term discovery on the MI355X (csrc/lalign.hip, cpc_local_align).

Given a corpus and no query, find the pairs of stretches that say the same thing, from the features alone (ZeroSpeech track 2):
a LOCAL alignment of every pair of utterances, with both ends free on both sides.  The reference has no such task.

The definition (include/cpc2_hip.h has the same text).  For a row item of n frames and a column item of m frames, d[i][j] is the
frame distance of cpc_abx_dtw, bit for bit (cosine: acos(clamp(<x_i, y_j>, -1, 1)) / pi on rows the caller normalised; euclidian:
||x_i - y_j||; f32, k-ordered fma chain).  Two f32 parameters: a threshold theta > 0 and a step penalty gamma >= 0.
    gain          g = theta - d[i][j]                                             (one f32 subtraction)
    candidates    diag H[i-1][j-1] (i > 0 and j > 0), left H[i][j-1] - gamma (j > 0), up H[i-1][j] - gamma (i > 0); the best is the
                  largest, ties to diag, then left, then up
    open          no candidate, or best <= 0:  h = g, length = 1, start = (i, j)
    continue      otherwise:  h = g + best (one f32 addition), length = pred.length + 1, start = pred.start
    clamp         h > 0: the cell holds (H = h, length, start); otherwise H = 0 and it carries nothing (a NaN distance closes it)
The result of a pair is the cell of largest H, among equals the smallest i, then the smallest j: score = H and
span = (start_i, end_i, start_j, end_j, length); score 0 and span -1 when no cell is positive; score NaN and span -1 when the
pair is not computable (an index or a length out of range).  Limits of this version: ONE match per pair; no band or slope
constraint other than gamma; items of at most MAX_FRAMES = 32767 frames.

plan_pairs lists every unordered pair once and cuts the list into segments of about equal numbers of cells with
term_detection.plan_segments; local_alignment runs cpc_local_align on it; select keeps and orders the matches; fragment_phones
and scores turn matches and frame labels into the normalised edit distance (NED) and the coverage.  Agreement of these two
numbers with the ZeroSpeech TDE toolkit is UNMEASURED: they follow its published definitions (30 ms / 50 % rule for the phones
of a fragment, NED as Levenshtein over the longer transcription), not its code, and its grouping, boundary and token / type
scores are not made.  There is no CPU path for the alignment: tensors must be on the GPU.
"""
import math

import numpy as np
import torch

from . import _lib
from . import term_detection as td
from .term_detection import COSINE, EUCLIDIAN, distance_code  # noqa: F401

MAX_FRAMES = 32767                 # the kernel's limit: the two start indices of a cell share one word
SPAN = 5                           # start_i, end_i, start_j, end_j, length


# --------------------------------------------------------------------------- planner
def plan_pairs(items, lens, exclude=None, cell_budget=None):
    """The kernel's work list on the host: every unordered pair of distinct items of `items` exactly once, the smaller index as
    the ROW item (a < b), without the pairs named in `exclude` ((a, b) in either order: pieces of one file, say), cut into
    segments even in cells by term_detection.plan_segments (cell_budget: see there).  lens: the length of every item.
    Returns (seg_a [S] int32, seg_start [S + 1] int32, pair_b [P] int32, pair_a [P] int32), pairs in ascending (a, b)."""
    items = np.unique(np.asarray(items, dtype=np.int64).reshape(-1))
    both = [(int(a), int(b)) for a, b in (exclude or ())]
    both += [(b, a) for a, b in both]
    rows = items[:-1]
    cols = [items[k + 1:] for k in range(len(rows))]
    seg_a, seg_start, pair_b, pair_row = td.plan_segments(rows, cols, lens, exclude=both, cell_budget=cell_budget)
    pair_a = rows[pair_row].astype(np.int32) if len(rows) else np.zeros(0, np.int32)
    return seg_a, seg_start, pair_b, pair_a


# --------------------------------------------------------------------------- kernel call
def run_segments(frames, item_off, item_len, seg_a, seg_start, pair_b, max_len_a, max_len_b, distance, theta, gamma, scratch=None):
    """cpc_local_align on a given work list (device int32 tensors): (score [P] f32, span [P, 5] int32: start_i, end_i, start_j,
    end_j, length).  scratch: a device buffer of at least cpc_local_align_scratch_bytes (default: the package's arena)."""
    frames, n_seg, n_pairs = td.check_work_list("term discovery", frames, item_off, item_len, seg_a, seg_start, pair_b,
                                                ("seg_a", "pair_b"))
    lib = _lib.load()
    return td._call_segments("term discovery", "cpc_local_align", lib.cpc_local_align_scratch_bytes, lib.cpc_local_align, "lalign",
                             (frames, frames.size(1)), (item_off, item_len, seg_a, seg_start, pair_b),
                             (n_seg, n_pairs, max_len_a, max_len_b), (int(distance), float(theta), float(gamma)), SPAN, scratch)


def _local_alignment(run, data, item_len, items, exclude, lens_host, cell_budget):
    """What local_alignment and local_alignment_units do once `data` (frames or units) is checked: the plan on the host, its
    upload, and run(seg_a, seg_start, pair_b, max_len_a, max_len_b), the run_segments of the kind."""
    lens = np.asarray(item_len.cpu().numpy() if lens_host is None else lens_host, dtype=np.int64)
    seg_a, seg_start, pair_b, pair_a = plan_pairs(items, lens, exclude, cell_budget)
    dev = data.device
    if pair_b.size == 0:
        return (torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, SPAN, dtype=torch.int32, device=dev), pair_a, pair_b)
    max_len_a = max(1, int(lens[seg_a].max()))
    max_len_b = max(1, int(lens[pair_b].max()))
    score, span = run(torch.from_numpy(seg_a).to(dev), torch.from_numpy(seg_start).to(dev), torch.from_numpy(pair_b).to(dev),
                      max_len_a, max_len_b)
    return score, span, pair_a, pair_b


def local_alignment(frames, item_off, item_len, items, distance, theta, gamma, exclude=None, lens_host=None, cell_budget=None):
    """The best local alignment of every pair of `items`.  frames [total_frames, dp] f32 (dp a multiple of 4, padding columns
    zero, rows normalised by the caller for the cosine distance), item_off / item_len int32: the device layout of
    ABXFeatureLoader.device_frames.  items, exclude, cell_budget: see plan_pairs.  distance: COSINE / EUCLIDIAN or their names.
    Returns (score [P] f32, span [P, 5] int32, pair_a [P], pair_b [P]): the first two on the device, the pair lists as int32
    numpy arrays (item indices, a < b; a is the row item: span = start_a, end_a, start_b, end_b, length)."""
    _lib.require_gpu(frames, item_off, item_len)
    if isinstance(distance, str):
        distance = distance_code(distance)
    return _local_alignment(lambda *work: run_segments(frames, item_off, item_len, *work, distance, theta, gamma), frames, item_len,
                            items, exclude, lens_host, cell_budget)


# --------------------------------------------------------------------------- quantized units (csrc/lalign_units.hip)
def run_segments_units(units, item_off, item_len, seg_a, seg_start, pair_b, max_len_a, max_len_b, d_same, d_diff, theta, gamma,
                       scratch=None):
    """cpc_local_align_units on a given work list (device int32 tensors): run_segments with the frames replaced by unit ids
    [total_frames] int32 and the distance by its two values (d_same between equal units, d_diff between different ones;
    abx_group_computation.unit_frame_distances makes them).  scratch: at least cpc_local_align_units_scratch_bytes."""
    n_seg, n_pairs = td.check_unit_work_list("term discovery on units", units, item_off, item_len, seg_a, seg_start, pair_b,
                                             ("seg_a", "pair_b"))
    lib = _lib.load()
    return td._call_segments("term discovery on units", "cpc_local_align_units", lib.cpc_local_align_units_scratch_bytes,
                             lib.cpc_local_align_units, "lalign_units", (units,), (item_off, item_len, seg_a, seg_start, pair_b),
                             (n_seg, n_pairs, max_len_a, max_len_b), (float(d_same), float(d_diff), float(theta), float(gamma)),
                             SPAN, scratch)


def local_alignment_units(units, item_off, item_len, items, d_same, d_diff, theta, gamma, exclude=None, lens_host=None,
                          cell_budget=None):
    """local_alignment on items of unit ids: units [total_frames] int32 on the device, d_same / d_diff the frame distance between
    equal / different units.  The same plan and the same returns."""
    td._check_units("term discovery on units", units, item_off, item_len)
    return _local_alignment(lambda *work: run_segments_units(units, item_off, item_len, *work, d_same, d_diff, theta, gamma), units,
                            item_len, items, exclude, lens_host, cell_budget)


# --------------------------------------------------------------------------- matches
def select(score, span, min_frames, min_score):
    """The pairs kept as matches: both sides span at least min_frames frames (end - start + 1) and the score is at least
    min_score (a pair without a positive cell or that was not computable is never kept).  Returns their indices as an int64 numpy
    array ordered by (-score, pair index)."""
    score = np.asarray(score.cpu() if isinstance(score, torch.Tensor) else score, dtype=np.float32).reshape(-1)
    span = np.asarray(span.cpu() if isinstance(span, torch.Tensor) else span, dtype=np.int64).reshape(-1, SPAN)
    with np.errstate(invalid="ignore"):
        keep = (span[:, 0] >= 0) & (score >= min_score) & (score > 0)
    keep &= (span[:, 1] - span[:, 0] + 1 >= min_frames) & (span[:, 3] - span[:, 2] + 1 >= min_frames)
    kept = np.flatnonzero(keep)
    return kept[np.argsort(-score[kept].astype(np.float64), kind="stable")]


def fragment_phones(labels, start, end):
    """The phone transcription of frames start .. end (both included) of a file with frame labels `labels`: the runs of equal
    labels of the file, a run being included when its overlap with the fragment is at least 3 frames (30 ms) or at least half of
    the run: the rule of the ZeroSpeech TDE evaluation."""
    labels = [int(x) for x in labels]
    out, at = [], 0
    while at < len(labels):
        stop = at
        while stop + 1 < len(labels) and labels[stop + 1] == labels[at]:
            stop += 1
        overlap = min(stop, end) - max(at, start) + 1
        if overlap >= 3 or (overlap > 0 and 2 * overlap >= stop - at + 1):
            out.append(labels[at])
        at = stop + 1
    return out


def edit_distances(seqs_a, seqs_b):
    """Levenshtein distance of each pair of label lists, on the device (cpc_align_score with d = m = -1, r = 0): a list of ints.
    Pairs of two empty sequences are not sent: their distance is 0."""
    from . import seq_alignment
    todo = [k for k, (a, b) in enumerate(zip(seqs_a, seqs_b)) if len(a) or len(b)]
    out = [0] * len(seqs_a)
    if not todo:
        return out
    dev = torch.device("cuda")

    def padded(seqs):
        width = max(1, max(len(s) for s in seqs))
        mat = np.zeros((len(seqs), width), dtype=np.int32)
        for k, s in enumerate(seqs):
            mat[k, :len(s)] = s
        return torch.from_numpy(mat).to(dev), torch.tensor([len(s) for s in seqs], dtype=torch.int32, device=dev)

    a, la = padded([seqs_a[k] for k in todo])
    b, lb = padded([seqs_b[k] for k in todo])
    dist = seq_alignment.align_score_batch(a, la, b, lb, -1, -1, 0).cpu().tolist()
    for k, v in zip(todo, dist):
        out[k] = int(v)
    return out


def scores(matches, labels, n_frames, distances=None):
    """NED and coverage of a list of matches.  matches: (file_a, start_a, end_a, file_b, start_b, end_b) with frames, ends included;
    labels: {file: frame labels} (a match with an unlabelled file is counted and left out of the NED); n_frames: {file: frames} of
    every searched utterance.
      NED       the mean over the matched pairs of levenshtein(phones_a, phones_b) / max(len_a, len_b), phones by fragment_phones;
                the edit distances come from the device (edit_distances; `distances`: one per match, when the caller has them), the
                quotients and their mean are taken on the host with math.fsum; pairs of two empty transcriptions are skipped and
                counted
      coverage  the frames of the searched utterances that lie in at least one fragment, over all their frames (two integers)
    and the number of matches, the mean fragment length in frames and the number of files with at least one fragment."""
    matches = [(fa, int(sa), int(ea), fb, int(sb), int(eb)) for fa, sa, ea, fb, sb, eb in matches]
    labelled = [k for k, m in enumerate(matches) if labels is not None and m[0] in labels and m[3] in labels]
    seqs_a = [fragment_phones(labels[matches[k][0]], matches[k][1], matches[k][2]) for k in labelled]
    seqs_b = [fragment_phones(labels[matches[k][3]], matches[k][4], matches[k][5]) for k in labelled]
    if distances is None:
        dist = edit_distances(seqs_a, seqs_b)
    else:
        dist = [int(distances[k]) for k in labelled]
    quotients, n_empty = [], 0
    for a, b, lev in zip(seqs_a, seqs_b, dist):
        if not a and not b:
            n_empty += 1
            continue
        quotients.append(lev / max(len(a), len(b)))
    covered = {name: np.zeros(int(n), dtype=bool) for name, n in n_frames.items()}
    lengths = []
    for fa, sa, ea, fb, sb, eb in matches:
        for name, s, e in ((fa, sa, ea), (fb, sb, eb)):
            lengths.append(e - s + 1)
            if name in covered:
                covered[name][max(0, s):e + 1] = True
    n_covered = int(sum(int(c.sum()) for c in covered.values()))
    total = int(sum(int(n) for n in n_frames.values()))
    return {"ned": math.fsum(quotients) / len(quotients) if quotients else float("nan"),
            "coverage": n_covered / total if total else float("nan"),
            "n_matches": len(matches), "n_ned_pairs": len(quotients), "n_empty_pairs": n_empty,
            "n_unlabelled_pairs": len(matches) - len(labelled), "covered_frames": n_covered, "total_frames": total,
            "mean_fragment_frames": math.fsum(lengths) / len(lengths) if lengths else float("nan"),
            "n_files_with_fragment": int(sum(1 for c in covered.values() if c.any())), "n_files": len(covered)}
