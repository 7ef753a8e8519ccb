"""ABX group scoring on the MI355X kernels -- cpc/eval/ABX/abx_group_computation.py of the reference, same names and
arguments.

The reference scores one triplet group at a time: a broadcast distance product, a copy to the host and a Cython DTW per
(x, a) and (x, b) pair, recomputing the (x, a) DTWs for every b.  Here get_abx_scores_dtw_on_group plans all triplets of an
iterator (same order, same random draws), deduplicates the (x item, y item) pairs of a chunk of triplets, and runs two
kernels per chunk: cpc_abx_dtw (frame distances + DTW of every pair) and cpc_abx_counts (the integer counts of
dxa < dxb and dxa == dxb per triplet).  The host forms theta from the counts with the reference's float32 arithmetic.
There is no CPU path: tensors must be on the GPU, and the scores are computed there whatever device the features are on.

A dataset of quantized units (abx_iterators.ABXUnitLoader: one unit id per frame) takes the same plan, pair lists and
counts, with cpc_abx_dtw_units in place of cpc_abx_dtw: the frame distance of two one-hot rows takes two values, computed
once on the host by unit_frame_distances, and the one-hot matrix is never built.
"""
import math

import numpy as np
import torch

from ... import _lib
from . import abx_iterators as abx_it

COSINE, EUCLIDIAN = 0, 1
# index-list entries (Nx*Na + Nx*Nb per triplet) per chunk of triplets; bounds the device memory of a chunk (index lists,
# pair lists and pair results: at most ~16 bytes per entry)
MAX_PAIRS_PER_CHUNK = 1 << 22
_DP_ALIGN = 4


def get_cosine_distance_batch(a1, a2, epsilon=1e-8):
    r"""[N1, S1, D] x [N2, S2, D] (normalised) -> [N1, N2, S1, S2] cosine distances acos(<a, b>) / pi.  As a
    `distance_function` argument it selects the DTW kernel's cosine distance; called directly it returns the whole
    distance tensor (for inspection; the scoring path never forms it)."""
    _lib.require_gpu(a1, a2)
    N1, S1, D = a1.size()
    N2, S2, D = a2.size()
    prod = (a1.view(N1, 1, S1, 1, D)) * (a2.view(1, N2, 1, S2, D))
    return torch.clamp(prod.sum(dim=4), -1, 1).acos() / math.pi


def get_euclidian_distance_batch(a1, a2):
    r"""[N1, S1, D] x [N2, S2, D] -> [N1, N2, S1, S2] euclidean distances; as a `distance_function` argument it selects
    the DTW kernel's euclidean distance."""
    _lib.require_gpu(a1, a2)
    N1, S1, D = a1.size()
    N2, S2, D = a2.size()
    diff = a1.view(N1, 1, S1, 1, D) - a2.view(1, N2, 1, S2, D)
    return torch.sqrt((diff**2).sum(dim=4))


def get_distance_function_from_name(name_str):
    if name_str == 'euclidian':
        return get_euclidian_distance_batch
    if name_str == 'cosine':
        return get_cosine_distance_batch
    raise ValueError("Invalid distance mode")


def _distance_code(distance_function):
    if distance_function is get_cosine_distance_batch:
        return COSINE
    if distance_function is get_euclidian_distance_batch:
        return EUCLIDIAN
    raise ValueError(f"ABX: unsupported distance_function {distance_function!r}: the DTW kernels implement "
                     "get_cosine_distance_batch and get_euclidian_distance_batch")


def check_dtw_group_validity(a, b, x):
    assert len(a.size()) == len(b.size())
    assert len(a.size()) == len(x.size())
    assert a.size(2) == x.size(2)
    assert a.size(2) == b.size(2)


# --------------------------------------------------------------------------- device item store
class _Items:
    """Items on the device: frames [total_frames, dp] (dp = D padded with zeros to a multiple of 4), frame offsets and
    lengths (int32), plus host copies of the lengths."""

    def __init__(self, frames, off, lens, lens_host):
        self.frames, self.off, self.lens = frames, off, lens
        self.lens_host = np.asarray(lens_host, dtype=np.int64)
        self.n = int(self.lens_host.shape[0])

    @property
    def device(self):
        return self.frames.device

    @staticmethod
    def from_padded(groups, device):
        """Items from padded [N, S, D] tensors and their sizes, in order."""
        D = groups[0][0].size(2)
        dp = -(-D // _DP_ALIGN) * _DP_ALIGN
        rows, offs, lens, base = [], [], [], 0
        for data, size in groups:
            N, S, _ = data.size()
            rows.append(data.reshape(N * S, D))
            sizes = [int(v) for v in size.tolist()]
            offs += [base + i * S for i in range(N)]
            lens += sizes
            base += N * S
        frames = torch.zeros(base, dp, dtype=torch.float32, device=device)
        frames[:, :D] = torch.cat(rows, 0).to(torch.float32)
        return _Items(frames, torch.tensor(offs, dtype=torch.int32, device=device),
                      torch.tensor(lens, dtype=torch.int32, device=device), lens)


class _UnitItems:
    """Items of unit ids on the device: units [total_frames] int32, frame offsets and lengths (int32), host copies of the
    lengths, and the two frame distances {distance code: (d_same, d_diff)} of unit_frame_distances."""

    def __init__(self, units, off, lens, lens_host, distances):
        self.units, self.off, self.lens = units, off, lens
        self.lens_host = np.asarray(lens_host, dtype=np.int64)
        self.n = int(self.lens_host.shape[0])
        self.distances = distances

    @property
    def device(self):
        return self.units.device


def unit_frame_distances(n_units, normalize, distance_function):
    """(d_same, d_diff): the frame distance between two equal and two different one-hot rows of n_units columns, in f32
    with the torch expressions the reference applies to them: the rows as a [1, 2, n_units] tensor through
    normalize_with_singularity when `normalize` (as ABXFeatureLoader does with feature_function's output), then the
    broadcast product / difference of get_cosine_distance_batch / get_euclidian_distance_batch.  On the host: two rows."""
    code = _distance_code(distance_function)
    rows = torch.zeros(1, 2, max(int(n_units), 2), dtype=torch.float32)
    rows[0, 0, 0] = 1
    rows[0, 1, 1] = 1
    if normalize:
        rows = abx_it.normalize_with_singularity(rows)
    a1 = a2 = rows.view(2, 1, -1)                         # two items of one frame
    N, S, D = a1.size()
    if code == COSINE:
        prod = (a1.view(N, 1, S, 1, D)) * (a2.view(1, N, 1, S, D))
        dist = torch.clamp(prod.sum(dim=4), -1, 1).acos() / math.pi
    else:
        diff = a1.view(N, 1, S, 1, D) - a2.view(1, N, 1, S, D)
        dist = torch.sqrt((diff**2).sum(dim=4))
    dist = dist.view(2, 2)
    return float(dist[0, 0]), float(dist[0, 1])


def _segment_lists(items, px, py):
    """The kernels' work list of the pairs (px[p], py[p]) (sorted by px) on the device: x item of every segment, CSR starts,
    y items, number of segments, and the longest x / y item."""
    dev = items.device
    seg_x, counts = np.unique(px, return_counts=True)
    seg_start = np.zeros(len(seg_x) + 1, dtype=np.int32)
    np.cumsum(counts, out=seg_start[1:])
    max_lx = int(items.lens_host[seg_x].max())
    max_ly = int(items.lens_host[np.unique(py)].max())
    return (torch.from_numpy(seg_x.astype(np.int32)).to(dev), torch.from_numpy(seg_start).to(dev),
            torch.from_numpy(np.ascontiguousarray(py, dtype=np.int32)).to(dev), len(seg_x), max_lx, max_ly)


def _dtw_pairs(items, px, py, code):
    """DTW of the pairs (px[p], py[p]) (item indices, sorted by px) on the device: (values [n] fp32, path lengths).  Items of
    unit ids go through cpc_abx_dtw_units with the two frame distances of `code`, frames through cpc_abx_dtw."""
    lib = _lib.load()
    if isinstance(items, _UnitItems):
        name, query, call = "cpc_abx_dtw_units", lib.cpc_abx_dtw_units_scratch_bytes, lib.cpc_abx_dtw_units
        head, params = (_lib.ptr(items.units),), items.distances[code]
    else:
        name, query, call = "cpc_abx_dtw", lib.cpc_abx_dtw_scratch_bytes, lib.cpc_abx_dtw
        head, params = (_lib.ptr(items.frames), items.frames.size(1)), (code,)
    dev = items.device
    n = int(px.shape[0])
    d_seg_x, d_seg_start, d_py, n_seg, max_lx, max_ly = _segment_lists(items, px, py)
    nbytes = query(n_seg, max_lx, max_ly)
    scratch = _lib.scratch(nbytes, dev, tag="abx") if nbytes else None
    out = torch.empty(n, dtype=torch.float32, device=dev)
    plen = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(call(*head, _lib.ptr(items.off), _lib.ptr(items.lens), items.n, _lib.ptr(d_seg_x), _lib.ptr(d_seg_start),
                    _lib.ptr(d_py), n_seg, max_lx, max_ly, *params, _lib.ptr(out), _lib.ptr(plen), _lib.ptr(scratch), nbytes,
                    _lib.stream_ptr(dev)), name)
    return out, plen


def _shape_keys(X, A, B, symmetric, n_items):
    """Pair keys (x_item * n_items + y_item) of G triplets of one shape: X [G, Nx], A [G, Na], B [G, Nb] item indices ->
    dxa keys [G, Nx*Na] (-1 = excluded diagonal) and dxb keys [G, Nx*Nb].  Symmetric (X is A): only j > i is a DTW of its
    own, (x_i, a_j); (j, i) reuses it, as dtw.pyx:dtw_batch mirrors."""
    G, nx = X.shape
    na = A.shape[1]
    if symmetric:
        i, j = np.meshgrid(np.arange(na), np.arange(na), indexing="ij")
        ka = X[:, np.minimum(i, j)] * n_items + A[:, np.maximum(i, j)]
        ka[:, i == j] = -1
    else:
        ka = X[:, :, None] * n_items + A[:, None, :]
    kb = X[:, :, None] * n_items + B[:, None, :]
    return ka.reshape(G, -1), kb.reshape(G, -1)


def _count_chunk(items, trips, symmetric, code):
    """Integer counts (lt, eq) of a chunk of triplets [(a_items, b_items, x_items)] through the two kernels, plus the
    number of unique pairs and of DTW cells."""
    dev = items.device
    by_shape = {}
    for t, (a, b, x) in enumerate(trips):
        by_shape.setdefault((len(x), len(a), len(b)), []).append(t)
    ka_l, kb_l, shape = [], [], np.zeros((len(trips), 5), dtype=np.int64)
    a_off = b_off = 0
    for (nx, na, nb), ts in by_shape.items():
        X = np.array([trips[t][2] for t in ts], dtype=np.int64)
        A = np.array([trips[t][0] for t in ts], dtype=np.int64)
        B = np.array([trips[t][1] for t in ts], dtype=np.int64)
        ka, kb = _shape_keys(X, A, B, symmetric, items.n)
        G = len(ts)
        shape[ts] = np.stack([np.full(G, nx), np.full(G, na), np.full(G, nb), a_off + np.arange(G) * ka.shape[1],
                              b_off + np.arange(G) * kb.shape[1]], axis=1)
        ka_l.append(ka.reshape(-1))
        kb_l.append(kb.reshape(-1))
        a_off += ka.size
        b_off += kb.size
    keys = np.concatenate(ka_l + kb_l)
    valid = keys >= 0
    uniq, inv = np.unique(keys[valid], return_inverse=True)
    idx = np.full(keys.shape[0], -1, dtype=np.int32)
    idx[valid] = inv
    px, py = uniq // items.n, uniq % items.n
    dist, _ = _dtw_pairs(items, px, py, code)
    d_idx_a = torch.from_numpy(idx[:a_off]).to(dev)
    d_idx_b = torch.from_numpy(idx[a_off:]).to(dev)
    d_shape = torch.from_numpy(shape.astype(np.int32)).to(dev)
    lt = torch.empty(len(trips), dtype=torch.int32, device=dev)
    eq = torch.empty(len(trips), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().cpc_abx_counts(_lib.ptr(dist), int(uniq.shape[0]), _lib.ptr(d_idx_a), _lib.ptr(d_idx_b),
                                          _lib.ptr(d_shape), len(trips), _lib.ptr(lt), _lib.ptr(eq),
                                          _lib.stream_ptr(dev)), "cpc_abx_counts")
    cells = int((items.lens_host[px] * items.lens_host[py]).sum())
    return lt, eq, int(uniq.shape[0]), cells


def theta_from_counts(lt, eq, na, nb, nx, symmetric):
    """theta = (lt + 0.5 * eq) / (n_pos * Nb) with the reference's float32 tensor arithmetic (abx_group_computation.py:
    79-95), element-wise over int64 CPU tensors; n_pos = Na (Na - 1) when symmetric, else Na Nx."""
    n_pos = na * (na - 1) if symmetric else na * nx
    sc = lt + 0.5 * eq
    return sc / (n_pos * nb)


def _score_triplets(items, trips, symmetric, code, max_pairs=MAX_PAIRS_PER_CHUNK, stats=None):
    """theta of every triplet [(a, b, x)], in chunks of at most max_pairs index entries (a triplet larger than that
    is a chunk of its own).  float32 CPU tensor."""
    lts, eqs, chunk, entries = [], [], [], 0
    n_pairs = n_cells = 0

    def flush():
        nonlocal n_pairs, n_cells
        lt, eq, npairs, cells = _count_chunk(items, chunk, symmetric, code)
        lts.append(lt)
        eqs.append(eq)
        n_pairs += npairs
        n_cells += cells

    for t in trips:
        e = len(t[2]) * (len(t[0]) + len(t[1]))
        if chunk and entries + e > max_pairs:
            flush()
            chunk, entries = [], 0
        chunk.append(t)
        entries += e
    if chunk:
        flush()
    lt = torch.cat(lts).cpu().to(torch.int64)
    eq = torch.cat(eqs).cpu().to(torch.int64)
    if stats is not None:
        stats["unique_pairs"] = stats.get("unique_pairs", 0) + n_pairs
        stats["chunks"] = stats.get("chunks", 0) + len(lts)
        stats["dtw_cells"] = stats.get("dtw_cells", 0) + n_cells
    na = torch.tensor([len(a) for a, _, _ in trips], dtype=torch.int64)
    nb = torch.tensor([len(b) for _, b, _ in trips], dtype=torch.int64)
    nx = torch.tensor([len(x) for _, _, x in trips], dtype=torch.int64)
    return theta_from_counts(lt, eq, na, nb, nx, symmetric)


# --------------------------------------------------------------------------- reference-shaped entry points
def get_distance_group_dtw(a1, a2, size1, size2, ignore_diag=False, symmetric=False,
                           distance_function=get_cosine_distance_batch):
    """[N1, N2] (CPU) normalised DTW distances between the items of two padded groups (abx_group_computation.py:44-60,
    dtw.pyx:dtw_batch): all (i, j), or j >= i mirrored when symmetric; the diagonal stays 0 with ignore_diag."""
    _lib.require_gpu(a1, a2)
    code = _distance_code(distance_function)
    N1, S1, D = a1.size()
    N2, S2, D = a2.size()
    assert size1.size(0) == N1
    assert size2.size(0) == N2
    items = _Items.from_padded([(a1, size1), (a2, size2)], a1.device)
    ii, jj = [], []
    for i in range(N1):
        for j in range(i if symmetric else 0, N2):
            if ignore_diag and i == j:
                continue
            ii.append(i)
            jj.append(j)
    out = torch.zeros((N1, N2))
    if not ii:
        return out
    ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
    vals, _ = _dtw_pairs(items, ii, N1 + jj, code)
    vals = vals.cpu()
    out[torch.from_numpy(ii), torch.from_numpy(jj)] = vals
    if symmetric:
        off = ii != jj
        out[torch.from_numpy(jj[off]), torch.from_numpy(ii[off])] = vals[torch.from_numpy(off)]
    return out


def get_theta_group_dtw(a, b, x, sa, sb, sx, distance_function, symmetric):
    """Share of (x, a, b) comparisons with DTW(x, a) < DTW(x, b), ties counting one half (abx_group_computation.py:
    63-95); symmetric: x is a, the diagonal excluded.  Same kernels as the batched path, on this one group."""
    check_dtw_group_validity(a, b, x)
    _lib.require_gpu(a, b, x)
    code = _distance_code(distance_function)
    if symmetric:
        items = _Items.from_padded([(x, sx), (b, sb)], x.device)
        nx = x.size(0)
        xs = list(range(nx))
        trip = (xs, list(range(nx, nx + b.size(0))), xs)
    else:
        items = _Items.from_padded([(x, sx), (a, sa), (b, sb)], x.device)
        nx, na = x.size(0), a.size(0)
        trip = (list(range(nx, nx + na)), list(range(nx + na, nx + na + b.size(0))), list(range(nx)))
    return _score_triplets(items, [trip], symmetric, code)[0].item()


def loc_dtw(data, distance_function, symmetric):
    coords, group_a, group_b, group_x = data
    group_a_data, group_a_size = group_a
    group_b_data, group_b_size = group_b
    group_x_data, group_x_size = group_x
    theta = get_theta_group_dtw(group_a_data, group_b_data, group_x_data, group_a_size, group_b_size, group_x_size,
                                distance_function, symmetric)
    return (coords, 1 - theta)


def plan_triplets(group_iterator):
    """(coords, [(a_items, b_items, x_items)]) of an iterator, in its order and with its random draws."""
    coords, trips = [], []
    for c, a, b, x in group_iterator.triplets():
        coords.append(c)
        trips.append((a, b, x))
    return coords, trips


def get_abx_scores_dtw_on_group(group_iterator, distance_function, symmetric, max_pairs=MAX_PAIRS_PER_CHUNK, stats=None):
    """Sparse tensor of 1 - theta over the iterator's board (abx_group_computation.py:98-129), computed in a few large
    launches over all its triplets.  max_pairs caps the index entries per chunk; `stats` (a dict) receives counters.
    A dataset of unit ids (ABXUnitLoader) goes through cpc_abx_dtw_units; everything else is the same code."""
    code = _distance_code(distance_function)
    coords, trips = plan_triplets(group_iterator)
    if not trips:
        raise ValueError("ABX: the item file yields no triplet for this mode (every (context, speaker) group holds a "
                         "single phone, or every phone a single item)")
    dataset = group_iterator.dataset
    device = torch.device("cuda", torch.cuda.current_device())
    if isinstance(dataset, abx_it.ABXUnitLoader):
        units, off, lens = dataset.device_units(device)
        items = _UnitItems(units, off, lens, [f[1] for f in dataset.features],
                           {code: unit_frame_distances(dataset.n_units, dataset.normalize, distance_function)})
    else:
        frames, off, lens = dataset.device_frames(device, -(-dataset.feature_dim // _DP_ALIGN) * _DP_ALIGN)
        items = _Items(frames, off, lens, [f[1] for f in dataset.features])
    with torch.no_grad():
        theta = _score_triplets(items, trips, symmetric, code, max_pairs, stats)
    values = (1 - theta.to(torch.float64)).to(torch.float32)
    if stats is not None:
        stats["triplets"] = stats.get("triplets", 0) + len(trips)
    return torch.sparse_coo_tensor(torch.LongTensor(coords).t(), values, group_iterator.get_board_size())
