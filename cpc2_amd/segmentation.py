"""Unsupervised phone segmentation and its scores on the device (csrc/segment.hip, include/cpc2_hip.h version 124; DESIGN.md
section 22).  The reference has no such tool, so the definition is the specification: the recipe of Kreuk et al. 2020 (a boundary
wherever consecutive frames stop resembling each other) scored by precision / recall / F1 / over-segmentation / R-value
(Rasanen et al. 2009) at a tolerance in frames.

One utterance has frames x[0..L) of D float32 columns, optional frame labels l[0..L') and thresholds p[0..K):
    d[t]    = 1 - dot(x_t, x_t+1) / sqrt(|x_t|^2 |x_t+1|^2), t < L - 1 (1 when the product of the squared norms is 0), the sums in
              float64.  A function of the two rows alone, symmetric in them: equal frame pairs give equal bits.
    peaks   of d as scipy.signal.find_peaks finds them (a plateau counts once, at its middle; the ends are never peaks), with
              the prominences of scipy.signal.peak_prominences (wlen=None)
    kept    at threshold p: prominence >= p * (max d - min d); a kept peak at q is a boundary at frame q + 1, (q + 1) * 10 ms
    ref     frames f in [1, n_l - 1] with l[f] != l[f-1], n_l = min(L, L'); hypotheses at frames >= n_l are dropped
    counts  per (utterance, threshold): n_hyp, hits (one-to-one matching by two pointers over the sorted lists), hyp_near (hypotheses
              with a reference within tol) and ref_near (references with a hypothesis within tol: the lenient counts of Kreuk et
              al.'s public scorer)
    scores  from integer totals (boundary_scores)
An utterance with a non-finite feature has status 2 and no boundaries; the others of its batch are unaffected.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr

MAX_THRESHOLDS = 64            # cpc_seg_boundaries: one lane per threshold
FRAME_SECONDS = 160 / 16000    # one frame of the encoder

SegResult = namedtuple("SegResult", ["n_peaks", "peaks", "prominences", "ranges", "counts", "status", "offsets", "lengths"])
SegResult.__doc__ = """find_boundaries' result, all on the device, for u utterances and K thresholds: n_peaks int32 [u]; peaks int32
and prominences float64 [total]: the peaks of utterance i in increasing order in the first n_peaks[i] slots at offsets[i] (the
other slots hold -1 / NaN); ranges float64 [u] (max d - min d); counts int32 [u, K, 4] = n_hyp, hits, hyp_near, ref_near; status
int32 [u] (0, or 2: a non-finite d or an invalid utterance, which has no peaks); offsets int64 [u] and lengths int32 [u] as given."""


def _tables(offsets, lengths, device):
    offsets = torch.as_tensor(offsets, dtype=torch.int64).to(device).contiguous()
    lengths = torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()
    if offsets.dim() != 1 or offsets.shape != lengths.shape or offsets.numel() == 0:
        raise ValueError(f"segmentation: offsets and lengths must be two equal non-empty vectors (got {tuple(offsets.shape)} and "
                         f"{tuple(lengths.shape)})")
    return offsets, lengths


def frame_dissimilarity(features, offsets=None, lengths=None, return_status=False):
    """The cosine dissimilarity of consecutive frames, float64 on the device.
      features [L, D]                       -> d [max(L - 1, 0)]
      features [b, L, D], lengths [b]       -> d [b, L]: row i holds lengths[i] - 1 values (lengths None: L everywhere)
      features [total, D] (rows may have a stride), offsets [u], lengths [u]: a packed buffer -> d [total], utterance i at
                                               offsets[i] .. offsets[i] + lengths[i] - 2
    Slots that hold no value are NaN.  return_status: (d, status int32 [utterances]), 2 for an utterance with a non-finite feature
    (its pairs with such a row are NaN) or whose rows leave the buffer."""
    require_gpu(features)
    if features.dtype != torch.float32:
        raise TypeError(f"cpc2_amd kernels are fp32 only (got {features.dtype})")
    dev = features.device
    shape = None
    if features.dim() == 3:
        if offsets is not None:
            raise ValueError("frame_dissimilarity: offsets belong to a packed [total, D] buffer, not to a [b, L, D] batch")
        b, L, D = features.shape
        shape = (b, L)
        offsets = torch.arange(b, dtype=torch.int64) * L
        lengths = torch.full((b,), L, dtype=torch.int32) if lengths is None else lengths
        rows = features.contiguous().view(b * L, D)
    elif features.dim() == 2:
        rows = features
        if offsets is None:
            if lengths is not None:
                raise ValueError("frame_dissimilarity: lengths without offsets on a [L, D] matrix")
            offsets, lengths = [0], [features.shape[0]]
            shape = "single"
    else:
        raise ValueError(f"frame_dissimilarity: features must be [L, D], [b, L, D] or a packed [total, D] (got {tuple(features.shape)})")
    total, D = rows.shape
    if D < 1:
        raise ValueError("frame_dissimilarity: no column (D = 0)")
    if rows.stride(1) != 1 or (total > 1 and rows.stride(0) < D):
        rows = rows.contiguous()
    ld = rows.stride(0) if total > 1 else D
    offsets, lengths = _tables(offsets, lengths, dev)
    if isinstance(shape, tuple) and lengths.shape != (shape[0],):
        raise ValueError(f"frame_dissimilarity: {shape[0]} utterances but lengths {tuple(lengths.shape)}")
    max_len = min(max(int(lengths.max()), 0), total)                    # (sizes the grid; a longer utterance leaves the buffer anyway)
    d = torch.full((max(total, 1),), float("nan"), dtype=torch.float64, device=dev)
    status = torch.empty(offsets.numel(), dtype=torch.int32, device=dev)
    check(_lib.load().cpc_seg_dissimilarity(ptr(rows), total, ld, D, ptr(offsets), ptr(lengths), offsets.numel(), max_len, ptr(d),
                                            ptr(status), stream_ptr(dev)), "seg_dissimilarity")
    d = d[:total]
    if shape == "single":
        d = d[:max(total - 1, 0)]
    elif shape is not None:
        d = d.view(shape)
    return (d, status) if return_status else d


def reference_boundaries(labels, n):
    """The frames f in [1, n - 1] with labels[f] != labels[f - 1], as an int32 array (host)."""
    n = int(n)
    lab = np.asarray(labels[:max(n, 0)])
    if n < 2:
        return np.zeros(0, np.int32)
    return (np.flatnonzero(lab[1:] != lab[:-1]) + 1).astype(np.int32)


def find_boundaries(d, offsets, lengths, prominences, ref=None, tol=2, limits=None):
    """Peaks, prominences and counts of a packed d (float64 [total] on the device, utterance i's lengths[i] - 1 values at
    offsets[i]; lengths are in FRAMES) for the thresholds `prominences` (1 .. 64 of them) -> SegResult.
    ref: one sorted sequence of reference boundary frames per utterance (host; None: no scoring, hits and the near counts are 0);
    limits: per utterance n_l, hypotheses at frames >= n_l are dropped (None: the utterance's length)."""
    require_gpu(d)
    if d.dtype != torch.float64 or d.dim() != 1:
        raise TypeError(f"find_boundaries: d must be a float64 vector (got {d.dtype} {tuple(d.shape)})")
    dev = d.device
    d = d.contiguous()
    offsets, lengths = _tables(offsets, lengths, dev)
    u = offsets.numel()
    thr = torch.as_tensor(np.asarray(prominences, dtype=np.float64).reshape(-1))
    k = thr.numel()
    if not 1 <= k <= MAX_THRESHOLDS:
        raise ValueError(f"find_boundaries: {k} prominence thresholds; between 1 and {MAX_THRESHOLDS} are supported")
    tol = int(tol)
    if tol < 0:
        raise ValueError(f"find_boundaries: tol={tol} must be >= 0")
    thr = thr.to(dev)
    ref_flat = ref_off = ref_cnt = lim = None
    total_ref = 0
    if ref is not None:
        if len(ref) != u:
            raise ValueError(f"find_boundaries: {u} utterances but {len(ref)} reference lists")
        lists = [np.asarray(r, dtype=np.int32).reshape(-1) for r in ref]
        cnt = np.array([len(r) for r in lists], dtype=np.int32)
        total_ref = int(cnt.sum())
        flat = np.concatenate(lists + [np.zeros(1, np.int32)])           # (never empty: a device pointer that is not NULL)
        ref_flat = torch.from_numpy(flat).to(dev)
        ref_off = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt[:-1], dtype=np.int64)]).astype(np.int64)).to(dev)
        ref_cnt = torch.from_numpy(cnt).to(dev)
    if limits is not None:
        lim = torch.as_tensor(np.asarray(limits, dtype=np.int32).reshape(-1)).to(dev)
        if lim.numel() != u:
            raise ValueError(f"find_boundaries: {u} utterances but {lim.numel()} limits")
    total = d.numel()
    n_peaks = torch.empty(u, dtype=torch.int32, device=dev)
    peaks = torch.full((max(total, 1),), -1, dtype=torch.int32, device=dev)
    proms = torch.full((max(total, 1),), float("nan"), dtype=torch.float64, device=dev)
    ranges = torch.empty(u, dtype=torch.float64, device=dev)
    counts = torch.empty(u, k, 4, dtype=torch.int32, device=dev)
    status = torch.empty(u, dtype=torch.int32, device=dev)
    check(_lib.load().cpc_seg_boundaries(ptr(d), total, ptr(offsets), ptr(lengths), u, ptr(thr), k, ptr(ref_flat), total_ref,
                                         ptr(ref_off), ptr(ref_cnt), ptr(lim), tol, ptr(n_peaks), ptr(peaks), ptr(proms),
                                         ptr(ranges), ptr(counts), ptr(status), stream_ptr(dev)), "seg_boundaries")
    return SegResult(n_peaks, peaks[:total], proms[:total], ranges, counts, status, offsets, lengths)


def select_boundaries(result, prominence, limits=None):
    """The boundary frames kept at one threshold, per utterance (a list of int arrays on the host), from a SegResult's peaks and
    prominences: prom >= prominence * range in float64, as the kernel compares; frames >= limits[i] dropped."""
    n_peaks, peaks, proms = result.n_peaks.cpu().numpy(), result.peaks.cpu().numpy(), result.prominences.cpu().numpy()
    ranges, offsets = result.ranges.cpu().numpy(), result.offsets.cpu().numpy()
    out = []
    for i in range(len(n_peaks)):
        lo = int(offsets[i])
        q, pr = peaks[lo:lo + n_peaks[i]], proms[lo:lo + n_peaks[i]]
        frames = q[pr >= np.float64(prominence) * ranges[i]].astype(np.int64) + 1
        if limits is not None:
            frames = frames[frames < int(limits[i])]
        out.append(frames)
    return out


def segment(features, offsets=None, lengths=None, prominence=0.05):
    """The boundary frames of every utterance at one prominence threshold: a list of int64 arrays (one array for an [L, D] matrix).
    An utterance with a non-finite feature has none."""
    d = frame_dissimilarity(features, offsets, lengths)
    single = features.dim() == 2 and offsets is None
    if features.dim() == 3:
        b, L = d.shape
        offsets = torch.arange(b, dtype=torch.int64) * L
        lengths = torch.full((b,), L, dtype=torch.int32) if lengths is None else lengths
        d = d.reshape(-1)
    elif single:
        offsets, lengths = [0], [features.shape[0]]
        d = torch.cat([d, d.new_full((min(features.shape[0], 1),), float("nan"))])
    frames = select_boundaries(find_boundaries(d, offsets, lengths, [prominence]), prominence)
    return frames[0] if single else frames


def boundary_scores(n_ref, n_hyp, hits, ref_hits=None):
    """{'precision', 'recall', 'f1', 'os', 'rval'} from integer totals, in Python floats: P = hits / n_hyp (0 when nothing is
    hypothesised), R = hits / n_ref (0 without references), F1 = 2 P R / (P + R) (0 when both are 0), OS = n_hyp / n_ref - 1 (NaN
    without references, and the R-value with it), r1 = sqrt((1 - R)^2 + OS^2), r2 = (R - 1 - OS) / sqrt(2),
    rval = 1 - (|r1| + |r2|) / 2.  ref_hits (the lenient scores): R = ref_hits / n_ref with P = hits / n_hyp, for hits = hyp_near
    and ref_hits = ref_near."""
    n_ref, n_hyp, hits = int(n_ref), int(n_hyp), int(hits)
    precision = hits / n_hyp if n_hyp else 0.0
    recall = (hits if ref_hits is None else ref_hits) / n_ref if n_ref else 0.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    over = n_hyp / n_ref - 1 if n_ref else float("nan")
    r1 = math.sqrt((1 - recall) ** 2 + over ** 2)
    r2 = (recall - 1 - over) / math.sqrt(2)
    return {"precision": precision, "recall": recall, "f1": f1, "os": over, "rval": 1 - (abs(r1) + abs(r2)) / 2}
