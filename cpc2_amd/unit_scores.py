"""Quantized units scored against frame-level phone labels (csrc/unit_scores.hip, include/cpc2_hip.h version 126; DESIGN.md
section 24): phone purity, cluster purity and PNMI (Hsu et al. 2021, HuBERT, section IV-A), the bitrate of the unit stream (Dunbar
et al. 2019, ZeroSpeech 2019), the run lengths of both streams, and the units' change points scored as phone boundaries.  The
reference has no counterpart, so the definition is the specification.

The device makes integers only (count): the joint table joint[z][y] of frames with unit z and phone y, the run starts of both
streams, and per utterance the boundary counts (n_ref, n_hyp, hits, hyp_near, ref_near) of segmentation.py at one tolerance.  The
scores are made from those integers on the host in float64 (scores), every sum through math.fsum over the cells in row-major
order: a score is a function of the integers alone.

With N = the number of frames, p(y, z) = joint[z][y] / N, log = log2:
    phone_purity   = sum_z max_y p(y, z)          cluster_purity = sum_y max_z p(y, z)
    H_phone, H_unit the entropies of the marginals; MI = sum p(y, z) log2(p(y, z) / (p(y) p(z))); pnmi = MI / H_phone
    perplexity     = 2 ** H_unit; used_units = units with a frame
    bitrate_frames = N H_unit / D and bitrate_runs = R H_runs / D bits per second, R = sum unit_runs, H_runs the entropy of
                     unit_runs / R, D = N * feature_size seconds
    mean_unit_run  = N / R and mean_phone_run = N / sum phone_runs, in frames
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import segmentation
from ._lib import check, ptr, require_gpu, stream_ptr

MAX_UNITS = 16384
MAX_PHONES = 1024
BOUNDARY_NAMES = ("n_ref", "n_hyp", "hits", "hyp_near", "ref_near")

UnitCounts = namedtuple("UnitCounts", ["joint", "unit_runs", "phone_runs", "invalid", "boundaries", "tol", "has_labels"])
UnitCounts.__doc__ = """count's result.  On the device: joint int64 [n_units, n_phones], unit_runs int64 [n_units], phone_runs int64
[n_phones], invalid int64 [1] (0: count raises otherwise).  boundaries: int64 [n, 5] on the host, one row (n_ref, n_hyp, hits,
hyp_near, ref_near) per utterance counted so far, in the order given; tol: the tolerance they were matched at; has_labels: False
when every frame was given the label 0."""


def _vector(t, dtype, name, device=None):
    t = torch.as_tensor(t)
    if device is not None:
        t = t.to(device)
    require_gpu(t)
    if t.dim() != 1:
        raise ValueError(f"unit_scores.count: {name} must be a vector (got {tuple(t.shape)})")
    return t.to(dtype).contiguous()


def count(units, labels, unit_offsets, label_offsets, lengths, n_units, n_phones, tol=2, into=None):
    """The integer tables of a batch of utterances -> UnitCounts.
    units int32 [words] and labels int32 [words'] (device): two packs; utterance i compares the lengths[i] frames at
    unit_offsets[i] and label_offsets[i] (the packs may have gaps and the utterances any order; words outside are never read).
    labels None: every frame has label 0, label_offsets is ignored and n_phones must be 1.
    into: an earlier UnitCounts of the same n_units, n_phones and tol.  Its tables are ADDED TO IN PLACE and returned in the new
    result: after the call the object passed as `into` is not to be used any more.
    Raises ValueError when a frame's unit is outside [0, n_units) or its label outside [0, n_phones), naming the first such
    utterance; the tables of `into` then hold the valid frames of this batch and are of no use."""
    require_gpu(units)
    dev = units.device
    units = _vector(units, torch.int32, "units")
    has_labels = labels is not None
    if has_labels:
        labels = _vector(labels, torch.int32, "labels", dev)
        label_offsets = _vector(label_offsets, torch.int64, "label_offsets", dev)
    else:
        label_offsets = None
    unit_offsets = _vector(unit_offsets, torch.int64, "unit_offsets", dev)
    lengths = _vector(lengths, torch.int32, "lengths", dev)
    u = lengths.numel()
    if unit_offsets.numel() != u or (has_labels and label_offsets.numel() != u):
        raise ValueError(f"unit_scores.count: {u} lengths but {unit_offsets.numel()} unit offsets"
                         + (f" and {label_offsets.numel()} label offsets" if has_labels else ""))
    n_units, n_phones, tol = int(n_units), int(n_phones), int(tol)
    if not 1 <= n_units <= MAX_UNITS or not 1 <= n_phones <= MAX_PHONES:
        raise ValueError(f"unit_scores.count: n_units={n_units} must be in 1 .. {MAX_UNITS} and n_phones={n_phones} in 1 .. {MAX_PHONES}")
    if not has_labels and n_phones != 1:
        raise ValueError(f"unit_scores.count: without labels every frame has label 0 and n_phones must be 1 (got {n_phones})")
    if tol < 0:
        raise ValueError(f"unit_scores.count: tol={tol} must be >= 0")
    if into is not None:
        if (tuple(into.joint.shape) != (n_units, n_phones) or into.tol != tol or into.has_labels != has_labels
                or into.joint.device != dev):
            raise ValueError("unit_scores.count: `into` was made with other n_units, n_phones, tol, labels or on another device")
        joint, unit_runs, phone_runs, invalid = into.joint, into.unit_runs, into.phone_runs, into.invalid
        earlier = into.boundaries
    else:
        joint = torch.zeros(n_units, n_phones, dtype=torch.int64, device=dev)
        unit_runs = torch.zeros(n_units, dtype=torch.int64, device=dev)
        phone_runs = torch.zeros(n_phones, dtype=torch.int64, device=dev)
        invalid = torch.zeros(1, dtype=torch.int64, device=dev)
        earlier = np.zeros((0, 5), np.int64)
    if u == 0:
        return UnitCounts(joint, unit_runs, phone_runs, invalid, earlier, tol, has_labels)
    host_lengths = lengths.cpu().numpy().astype(np.int64)
    if (host_lengths < 0).any():
        raise ValueError(f"unit_scores.count: utterance {int(np.flatnonzero(host_lengths < 0)[0])} has a negative length")
    total = int(host_lengths.sum())
    lib = _lib.load()
    need = max(lib.cpc_unit_counts_scratch_bytes(u), lib.cpc_unit_boundaries_scratch_bytes(u, total))
    if need == 0:
        check(-1, "unit_counts scratch query")
    out = torch.empty(u, 5, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        scratch = _lib.scratch(need, dev)
        args = (ptr(units), units.numel(), ptr(unit_offsets), ptr(labels), labels.numel() if has_labels else 0, ptr(label_offsets),
                ptr(lengths), u)
        check(lib.cpc_unit_counts(*args, n_units, n_phones, 0, ptr(joint), ptr(unit_runs), ptr(phone_runs), ptr(invalid),
                                  ptr(scratch), scratch.numel(), stream_ptr(dev)), "unit_counts")
        check(lib.cpc_unit_boundaries(*args, total, tol, ptr(out), ptr(scratch), scratch.numel(), stream_ptr(dev)), "unit_boundaries")
    if int(invalid.item()) != 0:
        raise ValueError(_first_invalid(units, labels, unit_offsets, label_offsets, host_lengths, n_units, n_phones,
                                        int(invalid.item())))
    rows = out.cpu().numpy().astype(np.int64)
    return UnitCounts(joint, unit_runs, phone_runs, invalid, np.concatenate([earlier, rows]), tol, has_labels)


def _first_invalid(units, labels, unit_offsets, label_offsets, lengths, n_units, n_phones, n_invalid):
    """The message of count's ValueError: the first utterance, in the order given, with a frame outside the tables (host)."""
    un, uo = units.cpu().numpy(), unit_offsets.cpu().numpy()
    la = labels.cpu().numpy() if labels is not None else None
    lo = label_offsets.cpu().numpy() if labels is not None else None
    for i, n in enumerate(lengths):
        n = int(n)
        if uo[i] < 0 or uo[i] + n > len(un) or (la is not None and (lo[i] < 0 or lo[i] + n > len(la))):
            return (f"unit_scores.count: {n_invalid} invalid frames; utterance {i} is the first: its {n} frames leave the pack")
        z = un[uo[i]:uo[i] + n]
        bad = (z < 0) | (z >= n_units)
        if la is not None:
            y = la[lo[i]:lo[i] + n]
            bad |= (y < 0) | (y >= n_phones)
        if bad.any():
            f = int(np.flatnonzero(bad)[0])
            return (f"unit_scores.count: {n_invalid} invalid frames; utterance {i} is the first: frame {f} has unit {int(z[f])}"
                    + (f" and label {int(la[lo[i] + f])}" if la is not None else "")
                    + f", outside n_units={n_units} / n_phones={n_phones}")
    return f"unit_scores.count: {n_invalid} invalid frames"


def _entropy(counts, total):
    """-sum p log2 p of the non-zero integer counts over their total, through fsum in the order given."""
    return -math.fsum((int(c) / total) * math.log2(int(c) / total) for c in counts if c) if total else 0.0


def _host(counts):
    if isinstance(counts.joint, torch.Tensor):
        return (counts.joint.cpu().numpy().astype(np.int64), counts.unit_runs.cpu().numpy().astype(np.int64),
                counts.phone_runs.cpu().numpy().astype(np.int64))
    return (np.asarray(counts.joint, dtype=np.int64), np.asarray(counts.unit_runs, dtype=np.int64),
            np.asarray(counts.phone_runs, dtype=np.int64))


def scores(counts, feature_size=0.01):
    """The scores of the module docstring from a UnitCounts (its tables on the device or as arrays), a dict of Python numbers.
    Without labels (counts.has_labels False) only the unit-side numbers: n_frames, n_units, used_units, H_unit, perplexity, the
    two bitrates, mean_unit_run.  With labels also the purities, H_phone, MI, pnmi (NaN when H_phone is 0), mean_phone_run, and
    `boundaries`: the summed integer counts with the strict and lenient scores of segmentation.boundary_scores."""
    feature_size = float(feature_size)
    if not feature_size > 0:
        raise ValueError(f"unit_scores.scores: feature_size={feature_size} must be positive")
    joint, unit_runs, phone_runs = _host(counts)
    n = int(joint.sum())
    if n == 0:
        raise ValueError("unit_scores.scores: no frame was counted")
    unit_tot = [int(v) for v in joint.sum(axis=1)]
    phone_tot = [int(v) for v in joint.sum(axis=0)]
    h_unit = _entropy(unit_tot, n)
    r = int(unit_runs.sum())
    h_runs = _entropy([int(v) for v in unit_runs], r)
    seconds = n * feature_size
    out = {"n_frames": n, "n_units": int(joint.shape[0]), "used_units": int(sum(1 for v in unit_tot if v)), "H_unit": h_unit,
           "perplexity": 2.0 ** h_unit, "bitrate_frames": n * h_unit / seconds, "bitrate_runs": r * h_runs / seconds,
           "mean_unit_run": n / r, "n_unit_runs": r}
    if not counts.has_labels:
        return out
    h_phone = _entropy(phone_tot, n)
    terms = []
    for z in range(joint.shape[0]):
        if not unit_tot[z]:
            continue
        for y in range(joint.shape[1]):
            c = int(joint[z, y])
            if c:
                # p(y, z) / (p(y) p(z)) = c n / (n_y n_z): ONE division of two exact integers
                terms.append((c / n) * math.log2((c * n) / (phone_tot[y] * unit_tot[z])))
    mi = math.fsum(terms)
    n_phone_runs = int(phone_runs.sum())
    out.update({"n_phones": int(joint.shape[1]),
                "phone_purity": math.fsum(int(joint[z].max()) / n for z in range(joint.shape[0])),
                "cluster_purity": math.fsum(int(joint[:, y].max()) / n for y in range(joint.shape[1])),
                "H_phone": h_phone, "MI": mi, "pnmi": mi / h_phone if h_phone > 0 else float("nan"),
                "mean_phone_run": n / n_phone_runs, "n_phone_runs": n_phone_runs})
    b = np.asarray(counts.boundaries, dtype=np.int64).reshape(-1, 5).sum(axis=0)
    n_ref, n_hyp, hits, hyp_near, ref_near = (int(v) for v in b)
    out["boundaries"] = {"tolerance": int(counts.tol), "n_ref": n_ref, "n_hyp": n_hyp, "hits": hits, "hyp_near": hyp_near,
                         "ref_near": ref_near, "strict": segmentation.boundary_scores(n_ref, n_hyp, hits),
                         "lenient": segmentation.boundary_scores(n_ref, n_hyp, hyp_near, ref_hits=ref_near)}
    return out


def unit_to_phone(counts):
    """Per used unit, in increasing order: (unit, majority phone, its count, the unit's frames, purity = count / frames); the
    lowest phone index wins a tie."""
    joint = _host(counts)[0]
    out = []
    for z in range(joint.shape[0]):
        tot = int(joint[z].sum())
        if tot:
            y = int(np.argmax(joint[z]))                 # (the first maximum: the lowest index)
            out.append((z, y, int(joint[z, y]), tot, int(joint[z, y]) / tot))
    return out
