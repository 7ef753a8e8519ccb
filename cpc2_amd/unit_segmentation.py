"""Duration-penalized unit segmentation (csrc/unit_dp.hip, include/cpc2_hip.h version 129): the unit
sequence that minimises the summed frame-to-code cost plus a charge `lambda` per segment -- the dynamic programme of Kamper & van
Niekerk (Interspeech 2021) with their linear duration penalty.  One parameter sweeps the ABX / bitrate curve of a fixed codebook.
The reference has no counterpart, so the definition is the specification:

    V[0][k] = (double) c[0][k]
    m[t]    = min_k V[t][k]          a[t] = the LOWEST k with V[t][k] == m[t]
    sw      = m[t-1] + lambda                                  (one f64 add)
    stay[t][k] = (V[t-1][k] <= sw)                             (a tie stays)
    V[t][k] = (double) c[t][k] + (stay[t][k] ? V[t-1][k] : sw) (one f64 add)
    u[T-1] = a[T-1];  u[t-1] = stay[t][u[t]] ? u[t] : a[t-1]

The cost matrix is opaque: kmeans_distances of a codebook, negative log posteriors, a probe's logits.  GPU tensors only.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr

MAX_UNITS = 16384
MAX_PENALTIES = 16
MAX_FRAMES = 1 << 24
DONE, EMPTY, NONFINITE, OUTSIDE = 0, 1, 2, 3


def check_penalties(penalties, who="segment_costs"):
    """The penalties as a list of floats: 1 .. 16 of them, each finite and >= 0."""
    pens = [float(v) for v in np.atleast_1d(np.asarray(penalties, dtype=np.float64))]
    if not 1 <= len(pens) <= MAX_PENALTIES:
        raise ValueError(f"{who}: {len(pens)} penalties; between 1 and {MAX_PENALTIES} go through one launch")
    for v in pens:
        if not (math.isfinite(v) and v >= 0):
            raise ValueError(f"{who}: penalty {v!r} must be finite and >= 0")
    return pens


def _vector(t, dtype, name, device):
    t = torch.as_tensor(t).to(device)
    if t.dim() != 1:
        raise ValueError(f"segment_costs: {name} must be a vector (got {tuple(t.shape)})")
    return t.to(dtype).contiguous()


def segment_costs(cost, offsets, lengths, penalties):
    """cost [n_rows, K] f32 (device, contiguous): a pack of rows; utterance i owns rows [offsets[i], offsets[i] + lengths[i]) (gaps
    and any order allowed).  penalties: 1 .. 16 finite values >= 0, all through ONE launch.
    -> (units [n_pen, n_rows] int32, energy [n_pen, n_utt] f64, n_segments [n_pen, n_utt] int32, status [n_pen, n_utt] int32), on
    the device.  units is -1 on rows no utterance owns and on those of an utterance with a non-finite cost (status 2); status 1:
    an empty utterance, 3: one that leaves the pack or has more than 2^24 frames."""
    require_gpu(cost)
    if cost.dtype != torch.float32:
        raise TypeError(f"cpc2_amd kernels are fp32 only (got {cost.dtype})")
    if cost.dim() != 2 or not cost.is_contiguous():
        raise ValueError(f"segment_costs: cost must be a contiguous [n_rows, K] matrix (got {tuple(cost.shape)}, contiguous: "
                         f"{cost.is_contiguous()})")
    n_rows, k = cost.shape
    if not 1 <= k <= MAX_UNITS:
        raise ValueError(f"segment_costs: K={k} must be in 1 .. {MAX_UNITS}")
    pens = check_penalties(penalties)
    dev = cost.device
    offsets = _vector(offsets, torch.int64, "offsets", dev)
    lengths = _vector(lengths, torch.int32, "lengths", dev)
    u = lengths.numel()
    if offsets.numel() != u:
        raise ValueError(f"segment_costs: {u} lengths but {offsets.numel()} offsets")
    n_pen = len(pens)
    units = torch.full((n_pen, n_rows), -1, dtype=torch.int32, device=dev)
    energy = torch.zeros(n_pen, u, dtype=torch.float64, device=dev)
    n_segments = torch.zeros(n_pen, u, dtype=torch.int32, device=dev)
    status = torch.zeros(n_pen, u, dtype=torch.int32, device=dev)
    if u == 0:
        return units, energy, n_segments, status
    host_len = lengths.cpu().numpy().astype(np.int64)
    total = int(np.clip(host_len, 0, MAX_FRAMES).sum())
    lib = _lib.load()
    need = lib.cpc_segment_units_scratch_bytes(u, total, k, n_pen)
    if need == 0:
        check(-1, "segment_units scratch query")
    pen_host = np.asarray(pens, dtype=np.float64)
    with torch.cuda.device(dev):
        scratch = _lib.scratch(need, dev)
        check(lib.cpc_segment_units(ptr(cost), n_rows, k, k, ptr(offsets), ptr(lengths), u, pen_host.ctypes.data, n_pen, ptr(units),
                              ptr(energy), ptr(n_segments), ptr(status), ptr(scratch), scratch.numel(), stream_ptr(dev)), "segment_units")
    return units, energy, n_segments, status


def segment_features(features, Ck, penalties):
    """One file: features [..., D] against the centroids Ck [..., K, D] -> (cost [n, K], units [n_pen, n] int32, energy [n_pen],
    n_segments [n_pen], status [n_pen]): kmeans_distances, then segment_costs on the whole matrix as one utterance."""
    from .clustering.clustering import kmeans_distances
    cost = kmeans_distances(features, Ck)
    n = cost.size(0)
    units, energy, n_segments, status = segment_costs(cost, torch.zeros(1, dtype=torch.int64), torch.tensor([n], dtype=torch.int32),
                                                      penalties)
    return cost, units, energy[:, 0], n_segments[:, 0], status[:, 0]


def runs(units, offsets, lengths):
    """Per utterance the runs of its unit stream, on the host: [(unit, start, length) int64 arrays], start counted from the
    utterance's first frame.  units: one int32 row of segment_costs' result (a tensor or an array)."""
    units = units.cpu().numpy() if isinstance(units, torch.Tensor) else np.asarray(units)
    if units.ndim != 1:
        raise ValueError(f"runs: units must be one row of the result (got {tuple(units.shape)})")
    offsets = offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)
    lengths = lengths.cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
    out = []
    for off, n in zip(offsets, lengths):
        off, n = int(off), int(n)
        if n <= 0 or off < 0 or off + n > len(units):
            out.append((np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)))
            continue
        z = units[off:off + n].astype(np.int64)
        start = np.concatenate([[0], np.flatnonzero(z[1:] != z[:-1]) + 1]).astype(np.int64)
        out.append((z[start], start, np.diff(np.concatenate([start, [n]])).astype(np.int64)))
    return out


def distortion(cost, units):
    """sum_t cost[t][units[t]] over the rows with units[t] >= 0, in f64 (a Python float).  For an utterance of status 0
        energy == distortion + lambda * (n_segments - 1)
    as real numbers; it is NOT asserted with ==, because the chain rounds once per frame in time order and a re-summation rounds
    differently."""
    require_gpu(cost, units)
    units = units.view(-1).long()
    if cost.dim() != 2 or units.numel() != cost.size(0):
        raise ValueError(f"distortion: cost {tuple(cost.shape)} against {units.numel()} units")
    keep = units >= 0
    picked = cost.double().gather(1, units.clamp(min=0).view(-1, 1)).view(-1)
    return float(torch.where(keep, picked, torch.zeros_like(picked)).sum().item())
